"""The contract of nrms_topk_sections_dot (include/nrms_hip.h) restated in numpy, for tests/test_topk_sections_host.py (its
self-checks) and tests/test_hip_topk_sections.py (the kernels).

Scores are formed in float64, which is exact for the integer lattices the tests use (|score| <= 9 d, far below 2^24), and rounded
to fp32 without loss; the prior is ONE fp32 addition to that score; a NaN sum removes the item; each section is ordered by
np.lexsort((ids, -scores)) (score descending, +inf first, equal scores by the smaller id, -0.0 == +0.0 and returned as +0.0) and
cut at k; the remaining slots hold id -1 / score -inf."""
import numpy as np


def topk_sections_ref(user, items, item_ids, section_ptr, k, exclude=None, bias=None):
    """user [B, d], items [N, d] fp32, item_ids [N], section_ptr [G + 1], exclude [B, n] ids or None, bias [N] fp32 BY ROW or
    None -> (scores [B, G, k] fp32, ids [B, G, k] int64)."""
    user, items = np.asarray(user, np.float32), np.asarray(items, np.float32)
    item_ids, section_ptr = np.asarray(item_ids), np.asarray(section_ptr)
    B, G = user.shape[0], len(section_ptr) - 1
    with np.errstate(invalid="ignore"):
        s = (user.astype(np.float64) @ items.astype(np.float64).T).astype(np.float32)
        if bias is not None:
            s = s + np.asarray(bias, np.float32)[None, :]              # one fp32 add (inf + -inf = NaN)
    s = np.where(s == 0, np.float32(0.0), s).astype(np.float32)        # -0.0 is +0.0
    out_s = np.full((B, G, k), -np.inf, np.float32)
    out_i = np.full((B, G, k), -1, np.int64)
    for b in range(B):
        for g in range(G):
            rows = np.arange(section_ptr[g], section_ptr[g + 1])
            ok = ~np.isnan(s[b, rows])
            if exclude is not None:
                ok &= ~np.isin(item_ids[rows], exclude[b])
            rows = rows[ok]
            top = rows[np.lexsort((item_ids[rows], -s[b, rows].astype(np.float64)))][:k]
            out_i[b, g, :len(top)] = item_ids[top]
            out_s[b, g, :len(top)] = s[b, top]
    return out_s, out_i
