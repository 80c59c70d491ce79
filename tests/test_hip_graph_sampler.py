"""Neighbour sampling from a device-resident click graph (click_graph.py, csrc/graphsample.hip) and the graph encoder on top of it
(model/graph_hip.py with an attached graph).  PARITY UNPINNED: the reference holds no graph model; the sampler is checked bit for
bit against the numpy restatement below of the five steps in include/nrms_hip.h (Philox4x32-7 in uint64 arithmetic, as
csrc/common.h: tests/philox_ref.py), the model against oracle/nrms_oracle.py + oracle/segpool_oracle.py with the out-of-batch rows
as constants."""
import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib, synth

from tests.philox_ref import philox4x32_7

pytestmark = pytest.mark.gpu

SITE = 5                                    # PHILOX_SITE_GRAPH_SAMPLE (csrc/common.h)
S32 = np.uint64(32)


# ---- numpy restatement ---------------------------------------------------------------------------------------------------------
def csr_ref(hist, n_news):
    """Grouping by hand: (user_ptr, user_news, news_ptr, news_users, n_padding, n_out_of_range)."""
    hist = np.asarray(hist, dtype=np.int64)
    per_user = [sorted({int(v) for v in row if 0 < v < n_news}) for row in hist]
    per_news = [[] for _ in range(n_news)]
    for u, row in enumerate(per_user):
        for j in row:
            per_news[j].append(u)
    flat = lambda lists: np.asarray([v for l in lists for v in l], dtype=np.int32)
    ptr = lambda lists: np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    return (ptr(per_user), flat(per_user), ptr(per_news), flat(per_news), int((hist == 0).sum()), int(((hist < 0) | (hist >= n_news)).sum()))


def sample_ref(g, slot_ids, K, seed):
    """The five steps of a draw.  g = (user_ptr, user_news, news_ptr, news_users) numpy; slot_ids [N] -> [N, K] int32."""
    user_ptr, user_news, news_ptr, news_users = (np.asarray(a).astype(np.int64) for a in g[:4])
    n_news, E = len(news_ptr) - 1, len(user_news)
    j = np.asarray(slot_ids, dtype=np.int64)[:, None]
    t = np.arange(K, dtype=np.int64)[None, :]
    ok = (j > 0) & (j < n_news)
    jj = np.where(ok, j, 0)
    r0, r1, _, _ = philox4x32_7(seed, (jj * K + t).astype(np.uint64), SITE)
    p0, deg = news_ptr[jj], news_ptr[jj + 1] - news_ptr[jj]
    ok = ok & (deg > 0) & (E > 0)
    if E == 0:
        return np.full((len(j), K), -1, dtype=np.int32)
    u = news_users[np.minimum(p0 + ((r0 * deg.astype(np.uint64)) >> S32).astype(np.int64), E - 1)]
    q0, du = user_ptr[u], user_ptr[u + 1] - user_ptr[u]
    m = user_news[np.minimum(q0 + ((r1 * du.astype(np.uint64)) >> S32).astype(np.int64), E - 1)]
    return np.where(ok & (m != j), m, -1).astype(np.int32)


def resolve_ref(slot_ids, nbr, cap, n_news):
    """(rows [N, K] int64, extra_ids [cap] int32, n_extra, n_dropped)."""
    slot_ids, nbr = np.asarray(slot_ids, dtype=np.int64), np.asarray(nbr, dtype=np.int64)
    N = len(slot_ids)
    first = np.full(n_news, -1, dtype=np.int64)
    live = np.flatnonzero((slot_ids > 0) & (slot_ids < n_news))
    first[slot_ids[live][::-1]] = live[::-1]                                   # the smallest slot wins
    valid = (nbr > 0) & (nbr < n_news)
    m = np.where(valid, nbr, 0)
    out = valid & (first[m] < 0)
    distinct = np.unique(nbr[out])
    rank = np.searchsorted(distinct, m)
    rows = np.where(valid, np.where(out, np.where(rank < cap, N + rank, -1), first[m]), -1)
    extra = np.zeros(cap, dtype=np.int32)
    keep = min(cap, len(distinct))
    extra[:keep] = distinct[:keep]
    return rows.astype(np.int64), extra, keep, len(distinct) - keep


# ---- graphs --------------------------------------------------------------------------------------------------------------------
def zipf_histories(n_users, H, n_news, seed, zipf=1.05, min_len=0):
    """[n_users, H] int64: left-aligned click lists of random length, news drawn with a Zipf skew (id 0 = padding)."""
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, n_news) ** zipf
    ids = rng.permutation(np.arange(1, n_news))[rng.choice(n_news - 1, size=(n_users, H), p=w / w.sum())]
    lens = rng.integers(min_len, H + 1, size=n_users)
    return np.where(np.arange(H)[None, :] < lens[:, None], ids, 0).astype(np.int64)


def build(hist, n_news):
    from pytorch_news_recommender_amd.click_graph import ClickGraph
    return ClickGraph.from_histories(torch.from_numpy(np.asarray(hist, dtype=np.int64)), n_news, "cuda")


def arrays(g):
    return tuple(a.cpu().numpy() for a in (g.user_ptr, g.user_news, g.news_ptr, g.news_users))


TOY = np.array([[1, 2, 3, 0], [2, 3, 0, 0], [4, 0, 0, 0], [1, 2, 4, 2]], dtype=np.int64)      # 5 news; news 0 is padding


# ---- 1. CSR build ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_users,H,n_news,seed", [(1, 1, 2, 0), (40, 7, 30, 1), (500, 50, 2000, 2), (3000, 20, 130000, 3)])
def test_csr_build_against_a_numpy_grouping(n_users, H, n_news, seed):
    rng = np.random.default_rng(seed + 100)
    hist = zipf_histories(n_users, H, n_news, seed)                            # duplicate clicks (Zipf), users without clicks (length 0)
    bad = rng.random(hist.shape) < 0.03                                        # ids out of range on both sides
    hist = np.where(bad, rng.choice([-1, -7, n_news, n_news + 5, 2 ** 40], size=hist.shape), hist)
    g = build(hist, n_news)
    up, un, npn, nu, n_pad, n_out = csr_ref(hist, n_news)
    assert (g.n_users, g.n_news, g.n_edges) == (n_users, n_news, len(un))
    assert g.n_padding == n_pad and g.n_out_of_range == n_out
    for got, want in zip(arrays(g), (up, un, npn, nu)):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    assert npn[1] == 0                                                          # id 0 is never an edge
    if n_news >= 2000:
        assert (np.diff(npn) == 0).sum() > 1                                    # unclicked news exist in these cases


# ---- 2. bit equality ---------------------------------------------------------------------------------------------------------------
def _slots(n_news, N, seed):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, n_news, size=N)
    s[rng.random(N) < 0.05] = 0
    return s.astype(np.int64)


@pytest.mark.parametrize("K", [1, 8, 33, 64])
@pytest.mark.parametrize("case", ["toy", "zipf130k", "single_click_users"])
def test_neighbor_ids_are_bit_equal_to_the_restatement(case, K):
    if case == "toy":
        hist, n_news, N = TOY, 5, 13
    elif case == "zipf130k":
        hist, n_news, N = zipf_histories(20000, 50, 130000, seed=5), 130000, 28160 + 37       # N not a multiple of 64
    else:
        hist, n_news, N = zipf_histories(300, 1, 400, seed=6, min_len=1), 400, 1001          # every user has ONE click: all draws -1
    g = build(hist, n_news)
    slot_ids = _slots(n_news, N, seed=K)
    slot_ids[:min(N, 5)] = [0, n_news + 3, -2, n_news, 1][:min(N, 5)]                       # padding, out of range (3 of them), id 1
    n_bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = g.sample_neighbors(torch.from_numpy(slot_ids).cuda(), K, seed=0xDEADBEEF12345678 + K, n_bad=n_bad)
    want = sample_ref(arrays(g), slot_ids, K, 0xDEADBEEF12345678 + K)
    assert got.dtype == torch.int32 and tuple(got.shape) == (N, K)
    assert np.array_equal(got.cpu().numpy(), want)
    assert int(n_bad.item()) == int(((slot_ids < 0) | (slot_ids >= n_news)).sum())
    deg = np.diff(arrays(g)[2])
    inside = (slot_ids > 0) & (slot_ids < n_news)
    assert (want[~inside] == -1).all() and (want[inside][deg[slot_ids[inside]] == 0] == -1).all()    # degree-0 news, padding, out of range
    if case == "single_click_users":
        assert (want == -1).all()
    if case == "zipf130k":
        assert (want >= 0).mean() > 0.3 and (deg[slot_ids[inside]] == 0).any()


# ---- 3. determinism ----------------------------------------------------------------------------------------------------------------
def test_two_calls_are_identical_rows_follow_their_slots_and_the_seed_matters():
    n_news, K = 5000, 8
    g = build(zipf_histories(2000, 30, n_news, seed=7), n_news)
    slot_ids = torch.from_numpy(_slots(n_news, 3000, seed=8)).cuda()
    a, b = g.sample_neighbors(slot_ids, K, seed=11), g.sample_neighbors(slot_ids, K, seed=11)
    assert torch.equal(a, b)
    perm = torch.randperm(3000, generator=torch.Generator().manual_seed(0)).cuda()
    assert torch.equal(g.sample_neighbors(slot_ids[perm], K, seed=11), a[perm])
    c = g.sample_neighbors(slot_ids, K, seed=12)
    assert (c != a).float().mean() > 0.2
    ra, rb = g.resolve_rows(slot_ids, a, 4096), g.resolve_rows(slot_ids, b, 4096)
    assert all(torch.equal(x, y) for x, y in zip(ra, rb))


# ---- 4. distribution ---------------------------------------------------------------------------------------------------------------
def test_neighbour_frequencies_follow_the_two_hop_distribution():
    """Over many seeds the draws of news j land on neighbour m with the exact two-hop probability
    p(m | j) = sum over clickers u of j of 1 / deg(j) * [m in news(u)] / deg(u) (m = j counts as "none"); every empirical
    frequency lies within 5 binomial standard deviations, 5 sqrt(p (1 - p) / n) (n = seeds x K draws; the bound is from n and p
    alone).  The seeds 0 .. 1999 were confirmed inside it with the restatement on the CPU (largest deviation 1.9 sd)."""
    hist = np.array([[1, 2, 3, 0], [2, 3, 0, 0], [4, 0, 0, 0], [1, 2, 4, 6], [5, 6, 2, 0], [6, 1, 0, 0]], dtype=np.int64)
    n_news, K, n_seeds = 8, 8, 2000
    g = build(hist, n_news)
    up, un, npn, nu = (a.astype(np.int64) for a in arrays(g))
    slot_ids = torch.arange(n_news, dtype=torch.int64, device="cuda")
    counts = np.zeros((n_news, n_news + 1), dtype=np.int64)                    # column n_news = "none"
    for seed in range(n_seeds):
        got = g.sample_neighbors(slot_ids, K, seed=seed).cpu().numpy()
        for j in range(n_news):
            counts[j] += np.bincount(np.where(got[j] < 0, n_news, got[j]), minlength=n_news + 1)
    n = n_seeds * K
    for j in range(n_news):
        p = np.zeros(n_news + 1)
        users = nu[npn[j]:npn[j + 1]]
        if len(users) == 0:
            p[n_news] = 1.0
        for u in users:
            for m in un[up[u]:up[u + 1]]:
                p[n_news if m == j else m] += 1.0 / (len(users) * (up[u + 1] - up[u]))
        assert abs(p.sum() - 1.0) < 1e-12
        dev = np.abs(counts[j] / n - p)
        bound = 5.0 * np.sqrt(p * (1.0 - p) / n)
        print("news %d: largest deviation %.2f sd" % (j, float((dev / np.maximum(bound / 5.0, 1e-300))[p * (1 - p) > 0].max(initial=0.0))))
        assert (dev <= bound).all(), (j, counts[j], p)


# ---- 5. resolve --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_news,N,K,cap_rule", [(5, 13, 3, "at"), (5000, 3001, 8, "at"), (5000, 3001, 8, "below"), (130000, 28160, 8, "above"),
                                                 (5000, 3001, 8, "zero")])
def test_rows_and_extra_ids_against_numpy(n_news, N, K, cap_rule):
    hist = TOY if n_news == 5 else zipf_histories(4000, 30, n_news, seed=9)
    g = build(hist, n_news)
    slot_np = _slots(n_news, N, seed=10)
    slot_ids = torch.from_numpy(slot_np).cuda()
    nbr = g.sample_neighbors(slot_ids, K, seed=3)
    nbr_np = nbr.cpu().numpy()
    n_distinct = resolve_ref(slot_np, nbr_np, 0, n_news)[3]
    assert n_distinct > 0 or n_news == 5
    cap = {"at": n_distinct, "below": max(n_distinct - 17, 1), "above": n_distinct + 100, "zero": 0}[cap_rule]
    dropped = torch.full((1,), 5, dtype=torch.int32, device="cuda")            # the counter accumulates
    rows, extra, n_extra = g.resolve_rows(slot_ids, nbr, cap, n_dropped=dropped)
    w_rows, w_extra, w_keep, w_dropped = resolve_ref(slot_np, nbr_np, cap, n_news)
    assert rows.dtype == torch.int64 and extra.dtype == torch.int32 and tuple(extra.shape) == (cap,)
    assert np.array_equal(rows.cpu().numpy(), w_rows)
    assert np.array_equal(extra.cpu().numpy(), w_extra)
    assert int(n_extra.item()) == w_keep and int(dropped.item()) == 5 + w_dropped
    if cap_rule == "at":
        assert w_dropped == 0 and (w_rows[nbr_np > 0] >= 0).all()               # at the cap nothing is dropped
    if cap_rule == "below":
        assert w_dropped == n_distinct - cap                                   # exactly the largest ids go
        gone = np.unique(nbr_np[(w_rows == -1) & (nbr_np > 0)])
        assert len(gone) == w_dropped and gone.min() > w_extra.max()
    inb = (w_rows >= 0) & (w_rows < N)
    assert (slot_np[w_rows[inb]] == nbr_np[inb]).all()                          # an in-batch row shows the neighbour's news


# ---- 6 .. 9: the model ----------------------------------------------------------------------------------------------------------
CASES = {
    # B, H, C, L, d, heads, q, K, kwargs: the geometries of tests/test_hip_graph.py
    "small": (6, 12, 4, 8, 64, 4, 32, 5, dict()),
    "empty_user_masked_cands": (5, 20, 5, 6, 64, 4, 32, 8, dict(empty_history_user=True, mask_some_candidates=True)),
    "one_neighbour_h40": (3, 40, 3, 5, 40, 2, 16, 1, dict()),
    "mind_dims": (4, 50, 5, 30, 300, 10, 200, 8, dict()),
}


def score_bar(fp16, scale):
    """Scores against the oracle (scale = max |oracle score| over the live candidates); tests/history.py imports it."""
    return (3e-4 if fp16 else 2e-5) * max(1.0, scale)


def grad_bound(ref, fp16, gscale):
    """Element-wise bound of |gradient - oracle| for one tensor (gscale: the largest oracle gradient outside the word table)."""
    rel = 2e-2 if fp16 else 1e-3
    # (d(W_K.bias) is identically zero in exact arithmetic -- softmax is shift-invariant -- so its bound is the noise term)
    return rel * np.abs(ref) + (rel * 0.5) * float(np.abs(ref).max()) + (1e-4 if fp16 else 2e-6) * gscale + 1e-9


def make_graph_model(shape, params, K, precision="fp32", cap=64):
    from pytorch_news_recommender_amd.config import Config
    from pytorch_news_recommender_amd.model.graph_hip import Model
    cfg = Config("graph")
    cfg.__nrms__()
    cfg.word_embed_size, cfg.num_attention_heads, cfg.query_vector_dim = shape.word_embed_size, shape.num_attention_heads, shape.query_vector_dim
    cfg.dropout, cfg.precision, cfg.graph_neighbors, cfg.graph_extra_rows = 0.0, precision, K, cap
    m = Model(cfg, pretrained_word_embedding=params["news_encoder.word_embedding.0.weight"])
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
    return m.to("cuda")


def make_world(case, seed=4, users=None):
    """A catalogue, the histories of 6 B users (the click graph) and a batch of B of them (default: the first B), with news ids."""
    B, H, Cn, L, d, h, q, K, kw = CASES[case]
    shape = synth.Shape(n_words=200, word_embed_size=d, num_attention_heads=h, query_vector_dim=q, batch_size=B, history_len=H,
                        n_candidates=Cn, n_words_title=L)
    rng = np.random.default_rng(seed)
    n_news = 4 * B * (H + Cn)
    titles = rng.integers(1, shape.n_words, size=(n_news, L)).astype(np.int64)
    titles[np.arange(L)[None, :] >= rng.integers(1, L + 1, size=n_news)[:, None]] = 0
    titles[0] = 0
    hist = zipf_histories(6 * B, H, n_news, seed + 1, zipf=0.9, min_len=2)
    if kw.get("empty_history_user"):
        hist[1] = 0
    users = np.arange(B) if users is None else np.asarray(users)
    bi = hist[users]
    ci = rng.integers(1, n_news, size=(6 * B, Cn)).astype(np.int64)[users]
    ci[:, 0] = hist[(users + 1) % len(hist), 0]                                 # a clicked news among the candidates
    cm = np.ones((B, Cn), dtype=np.uint8)
    if kw.get("mask_some_candidates"):
        cm[0, -2:] = 0
        ci[0, -2:] = 0
    batch = dict(browsed_ids=bi, browsed_mask=(bi != 0).astype(np.uint8), browsed_titles=titles[bi], candidate_ids=ci,
                 candidate_titles=titles[ci], candidate_mask=cm)
    return shape, synth.make_params_graph(shape, seed=3), titles, hist, batch, K, n_news


def tbatch(batch):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in batch.items()}


def expected_neighbors(g, batch, K, seed, cap, n_news):
    slot_ids = np.concatenate([np.where(batch["browsed_mask"] != 0, batch["browsed_ids"], 0).reshape(-1), batch["candidate_ids"].reshape(-1)])
    return resolve_ref(slot_ids, sample_ref(arrays(g), slot_ids, K, seed), cap, n_news)


def oracle_scores(pt, batch, titles, rows, extra_ids, n_extra, h):
    """nrms_oracle.news_encoder -> g = n + segment_pool over [n ; constants] -> h = segment_pool over clicked slots -> click_scores."""
    from oracle import nrms_oracle as orc
    from oracle import segpool_oracle as so
    bt, ct = torch.as_tensor(batch["browsed_titles"]).long(), torch.as_tensor(batch["candidate_titles"]).long()
    B, H, L = bt.shape
    C = ct.shape[1]
    N = B * (H + C)
    nv = orc.news_encoder(pt, torch.cat([bt.reshape(B * H, L), ct.reshape(B * C, L)], 0), h)
    with torch.no_grad():
        const = orc.news_encoder(pt, torch.as_tensor(titles[extra_ids]).long(), h)           # [cap, d] constants; rows past n_extra unused
    x = torch.cat([nv, const.detach()], 0)
    lv = lambda m: (pt[m + ".linear.weight"], pt[m + ".linear.bias"], pt[m + ".attention_query_vector"])
    ptr, idx = [0], []
    for r in range(N):
        idx += [int(v) for v in rows[r] if 0 <= int(v) < N + len(extra_ids)]
        ptr.append(len(idx))
    g = nv + so.segment_pool(x, *lv("neighbor_attention"), ptr, idx)
    valid = batch["browsed_mask"]
    ptr, idx = [0], []
    for b in range(B):
        idx += [b * H + k for k in range(H) if valid[b][k]]
        ptr.append(len(idx))
    hh = so.segment_pool(g, *lv("user_attention"), ptr, idx)
    return orc.click_scores(g[B * H:].view(B, C, -1), hh, torch.as_tensor(batch["candidate_mask"]))


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "fp16"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_scores_and_every_gradient_against_the_oracle_with_out_of_batch_neighbours(case, precision):
    from oracle import nrms_oracle as orc
    shape, params, titles, hist, batch, K, n_news = make_world(case)
    B, Cn, h = shape.batch_size, shape.n_candidates, shape.num_attention_heads
    g = build(hist, n_news)
    # room for every out-of-batch neighbour of the training draw and of the evaluation draw below, and a few unused rows
    cap = 5 + max(expected_neighbors(g, batch, K, seed, 1 << 20, n_news)[2] for seed in (0, 0x6A09E667F3BCC908))
    model = make_graph_model(shape, params, K, precision, cap).train()
    assert model.EVAL_SEED == 0x6A09E667F3BCC908
    model.attach_click_graph(g, torch.from_numpy(titles))
    rows, extra_ids, n_extra, dropped = expected_neighbors(g, batch, K, 0, cap, n_news)      # the first training batch: seed 0
    N = B * (shape.history_len + Cn)
    assert n_extra >= 1 and (rows >= N).any() and dropped == 0, "the case must have out-of-batch neighbours"
    dscores = (np.random.default_rng(5).standard_normal((B, Cn)) * 0.1).astype(np.float32)
    pt = orc.to_torch(params, requires_grad=True)
    s = oracle_scores(pt, batch, titles, rows, extra_ids, n_extra, h)
    live_t = torch.as_tensor(batch["candidate_mask"]) != 0
    (torch.where(live_t, s, torch.zeros_like(s)) * torch.from_numpy(dscores)).sum().backward()
    o_scores = s.detach().numpy()
    model.zero_grad()
    scores = model(tbatch(batch))
    scores.backward(torch.from_numpy(dscores).cuda())
    assert model.check_click_graph() == 0
    got = scores.detach().cpu().numpy()
    live = batch["candidate_mask"] != 0
    assert np.all(got[~live] == np.float32(-1e9))
    err, scale = float(np.abs(got - o_scores)[live].max()), float(np.abs(o_scores[live]).max())
    fp16 = precision == "fp16"
    print("graph+global %-24s %-6s scores err %.2e (scale %.2f), %d out-of-batch rows" % (case, precision, err, scale, n_extra))
    assert err <= score_bar(fp16, scale)
    named = dict(model.named_parameters())
    gscale = max(float(np.abs(v.grad.numpy()).max()) for k, v in pt.items() if not k.endswith("word_embedding.0.weight"))
    for n, v in pt.items():
        ref = v.grad.numpy()
        gr = named[n].grad.detach().cpu().numpy()
        bound = grad_bound(ref, fp16, gscale)
        print("      %-58s err %.2e  scale %.2e" % (n, float(np.abs(gr - ref).max()), float(np.abs(ref).max())))
        assert float((np.abs(gr - ref) - bound).max()) <= 0.0, (case, precision, n, float(np.abs(gr - ref).max()), float(np.abs(ref).max()))
    # inference: the eval-mode forward draws with EVAL_SEED; it must equal the training-path forward of the same neighbours
    # (explicit neighbor_rows / neighbor_vectors keys, the catalogue the model holds) at the file's inference bar
    model.eval()
    with torch.no_grad():
        inf = model(tbatch(batch)).cpu().numpy()
    e_rows, e_extra, e_n, _ = expected_neighbors(g, batch, K, model.EVAL_SEED, cap, n_news)
    explicit = dict(tbatch(batch), neighbor_rows=torch.from_numpy(e_rows),
                    neighbor_vectors=model._catalogue.index_select(0, torch.from_numpy(e_extra).long().cuda()))
    model.train()
    got2 = model(explicit).detach().cpu().numpy()
    assert float(np.abs(inf - got2)[live].max()) <= (3e-4 if fp16 else 1e-6) * max(1.0, scale)


def test_a_batch_without_the_key_is_unchanged_and_missing_ids_are_named():
    shape, params, titles, hist, batch, K, n_news = make_world("small")
    plain = synth.make_batch_graph(shape, K, seed=4)
    a = make_graph_model(shape, params, K).eval()
    b = make_graph_model(shape, params, K).eval()
    b.attach_click_graph(build(hist, n_news), torch.from_numpy(titles))
    with torch.no_grad():
        assert torch.equal(a(tbatch(plain)), b(tbatch(plain)))                  # explicit neighbor_rows: the graph is not consulted
        no_ids = {k: v for k, v in tbatch(batch).items() if k not in ("browsed_ids", "candidate_ids")}
        with pytest.raises(KeyError, match="browsed_ids.*candidate_ids"):
            b(no_ids)
    with pytest.raises(_lib.NrmsError, match="titles"):
        b.attach_click_graph(build(hist, n_news), torch.from_numpy(titles[:-1]))


def test_evaluation_scores_depend_on_the_user_alone():
    """User 0 scored next to two different sets of other users: with the global graph the two scores agree within the inference
    bar of the oracle test (1e-6 max(1, scale), fp32); with the batch-induced host sampler they do not -- the neighbours
    change with the batch."""
    case = "small"
    B = CASES[case][0]
    shape, params, titles, hist, batch_a, K, n_news = make_world(case, users=np.arange(B))
    batch_b = make_world(case, users=np.concatenate([[0], np.arange(B, 2 * B - 1)]))[4]
    batch_b["candidate_ids"][0], batch_b["candidate_titles"][0] = batch_a["candidate_ids"][0], batch_a["candidate_titles"][0]
    model = make_graph_model(shape, params, K, cap=512).eval()
    with torch.no_grad():
        ia, ib = model(tbatch(batch_a))[0].cpu().numpy(), model(tbatch(batch_b))[0].cpu().numpy()
        model.attach_click_graph(build(hist, n_news), torch.from_numpy(titles))
        ga, gb = model(tbatch(batch_a))[0].cpu().numpy(), model(tbatch(batch_b))[0].cpu().numpy()
    assert model.check_click_graph() == 0
    bar = 1e-6 * max(1.0, float(np.abs(ga).max()))
    print("user 0 in two batches: global |diff| %.2e, induced |diff| %.2e, bar %.2e" % (np.abs(ga - gb).max(), np.abs(ia - ib).max(), bar))
    assert float(np.abs(ga - gb).max()) <= bar
    assert float(np.abs(ia - ib).max()) > bar


def _synthetic_setup(n_users=96, n_imps=64, batch=32):
    from pytorch_news_recommender_amd.config import Config
    from pytorch_news_recommender_amd.data_handler import DeviceFeed, SyntheticMind
    from pytorch_news_recommender_amd.model.graph_hip import Model
    cfg = Config("graph_T")
    cfg.__nrms__()
    # (8 000 words: no word occurs more than 64 times in a 32-user batch -- see the repeatability test below)
    cfg.n_words, cfg.n_words_title, cfg.word_embed_size, cfg.num_attention_heads, cfg.query_vector_dim = 8000, 12, 64, 4, 32
    cfg.batch_size, cfg.max_candidate_size, cfg.graph_extra_rows = batch, 40, 4096
    corpus = SyntheticMind(cfg, n_news=600, seed=0)
    kw = dict(id2title_dict=corpus.id2title_dict, id2abst_dict=corpus.id2abst_dict, batch_size=batch, device="cuda")
    train_feed = DeviceFeed(cfg, corpus.train_samples(n_users), type=0, **kw)
    dev_samples, dev_labels = corpus.eval_samples(n_imps)
    dev_feed = DeviceFeed(cfg, dev_samples, type=1, **kw)

    def model():
        torch.manual_seed(7)
        m = Model(cfg, pretrained_word_embedding=corpus.embedding_table(cfg.word_embed_size)).to("cuda")
        m.attach_click_graph(train_feed.click_graph(), train_feed.titles)
        return m
    return cfg, train_feed, dev_feed, dev_labels, model


def test_device_feed_click_graph_has_one_user_per_distinct_history():
    cfg, train_feed, _, _, _ = _synthetic_setup()
    g = train_feed.click_graph()
    hist = train_feed.packed["hist"].cpu().numpy()
    distinct = np.unique(hist, axis=0)
    assert g.n_users == len(distinct) and g.n_news == train_feed.titles.shape[0] and g is train_feed.click_graph()
    want = csr_ref(distinct, g.n_news)
    for got, w in zip(arrays(g), want[:4]):
        assert np.array_equal(got, w)


def test_evaluate_twice_gives_one_auc_and_identical_train_steps_give_identical_parameters():
    """Bit equality of EVERY parameter after two identical train steps.  The library states one limit to that guarantee, and it
    is not the sampler's: the embedding-table gradient (csrc/embed.hip, scatter_grouped_kernel) sums a word's occurrences in
    64-entry chunks whose membership follows the order in which the placement's integer atomics resolve, so the gradient row of
    a word that occurs MORE than 64 times in a step is reproducible only up to the order of its chunks -- a last-bit difference
    that shows now and then.  With a 500-word vocabulary this test's second batch held one such word (71 occurrences) and the
    comparison of m1._flat with m2._flat failed intermittently on that table row.  The vocabulary is therefore large enough
    that every word stays inside the documented guarantee, and the test asserts that precondition on its own batches."""
    from pytorch_news_recommender_amd.train_eval import evaluate
    cfg, train_feed, dev_feed, dev_labels, make = _synthetic_setup()
    m = make()
    a1 = evaluate(cfg, m, dev_feed, dev_labels, verbose=False)
    a2 = evaluate(cfg, m, dev_feed, dev_labels, verbose=False)
    assert a1 == a2 and 0.0 < a1 < 1.0
    s1 = m.last_eval_scores.clone()
    evaluate(cfg, m, dev_feed, dev_labels, verbose=False)
    assert torch.equal(s1, m.last_eval_scores)
    batches = list(train_feed)[:2]
    for b in batches:
        words = torch.cat([b["browsed_titles"].reshape(-1), b["candidate_titles"].reshape(-1)])
        assert int(torch.bincount(words[words > 0]).max()) <= 64, "a word beyond the table gradient's bit-reproducible bucket size"
    m1, m2 = make().train(), make().train()
    for b in batches:
        m1.train_step(b)
        m2.train_step(b)
    torch.cuda.synchronize()
    for n in m1._names:                                                         # (named, so that a failure says which tensor)
        assert torch.equal(m1._layout.view(m1._flat, n), m2._layout.view(m2._flat, n)), n
    assert torch.equal(m1._flat, m2._flat)
    assert not torch.equal(m1._flat, make()._flat)                              # ... and the steps did move them
    assert m1.check_click_graph() == 0


def test_staleness_rule():
    cfg, train_feed, dev_feed, _, make = _synthetic_setup()
    cfg.dropout = 0.0
    m = make().train()
    batches = list(train_feed)
    old = m._catalogue.clone()
    m.train_step(batches[0])
    assert m._catalogue_stale and torch.equal(m._catalogue, old)                # training does not refresh
    step = m._graph_step
    assert step == 1                                                            # the train-step counter: one batch trained on
    with torch.no_grad():
        t_old = m(batches[1])                                                   # a training forward before the refresh: old vectors
    assert torch.equal(m._catalogue, old) and m._catalogue_stale
    assert m._graph_step == step                                                # a forward under no_grad is not a train step
    m.eval()
    dev_batch = next(iter(dev_feed))
    with torch.no_grad():
        e_lazy = m(dev_batch)                                                   # the first eval forward after the step refreshes
    assert not m._catalogue_stale and not torch.equal(m._catalogue, old)
    lazy = m._catalogue.clone()
    m.refresh_neighbor_vectors()
    assert torch.equal(m._catalogue, lazy)
    with torch.no_grad():
        assert torch.equal(m(dev_batch), e_lazy)                                # = a forward after an explicit refresh
    m.train()
    m._graph_step = step                                                        # the same draws as t_old
    with torch.no_grad():
        t_new = m(batches[1])
    assert not torch.equal(t_new, t_old)                                        # the refreshed vectors do reach a training forward
    m._catalogue, m._graph_step = old, step
    with torch.no_grad():
        assert torch.equal(m(batches[1]), t_old)                                # ... and t_old was computed from the old ones


# ---- 10. entry point ---------------------------------------------------------------------------------------------------------------
def test_run_v0_with_the_global_graph(tmp_path, monkeypatch):
    import os
    from pytorch_news_recommender_amd import run_v0, train_eval
    monkeypatch.chdir(tmp_path)
    real_train = run_v0.train

    def train_and_save(config, model, *a, **kw):
        # train() writes a checkpoint only when the dev AUC passes the reference's 0.56 (train_eval.py:59), which five steps may
        # not reach: write one through the same _save whatever the AUC, so that the checkpoint's keys are always checked
        hist = real_train(config, model, *a, **kw)
        hist["forced_ckpt"] = train_eval._save(config, model, len(hist["losses"]), 0.0)
        return hist
    monkeypatch.setattr(run_v0, "train", train_and_save)
    hist = run_v0.main(["--model", "graph", "--dataset", "synthetic", "--graph", "global", "--epochs", "1", "--synthetic_users", "192",
                        "--batch_size", "32", "--max_batches", "5", "--num_workers", "0", "--description", "T",
                        "--data_path", str(tmp_path / "data_processed"), "--save_path", str(tmp_path / "save")])
    assert len(hist["losses"]) == 5 and np.isfinite(hist["losses"]).all()
    assert hist["aucs"] and 0.0 < hist["aucs"][-1][1] < 1.0
    ckpts = [f for f in os.listdir(tmp_path / "save") if f.endswith(".ckpt")]
    assert hist["forced_ckpt"] in ckpts
    for f in ckpts:
        sd = torch.load(os.path.join(tmp_path / "save", f), map_location="cpu", weights_only=True)
        assert "model.neighbor_attention.linear.weight" in sd and "model.news_encoder.word_embedding.0.weight" in sd
    with pytest.raises(SystemExit):
        run_v0.main(["--model", "graph", "--dataset", "synthetic", "--graph", "global", "--recommend", "5"])
