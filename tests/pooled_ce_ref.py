"""numpy float64 restatement of nrms_pooled_ce_fwd_bwd (include/nrms_hip.h): the in-batch sampled softmax over the batch's shared
candidate pool.  Nothing here is shared with the kernels; tests/test_pooled_ce_host.py checks it against torch autograd."""
import numpy as np


def inclusion(B, C, cand_id, cand_mask=None, reject=None):
    """bool [B, M]: column j is in the softmax of row b.  cand_id [M] int64, cand_mask [M] or None, reject [B, R] or None."""
    M = B * C
    cand_id = np.asarray(cand_id).reshape(M)
    live = np.ones(M, dtype=bool) if cand_mask is None else np.asarray(cand_mask).reshape(M) != 0
    own = np.arange(B) * C
    inc = live[None, :] & (cand_id[None, :] != cand_id[own][:, None])
    if reject is not None and np.asarray(reject).size:
        rej = np.asarray(reject).reshape(B, -1)
        hit = (cand_id[None, :, None] == rej[:, None, :]) & (rej[:, None, :] > 0)
        inc &= ~hit.any(-1)
    inc[np.arange(B), own] = True
    inc[~live[own]] = False                       # a dead row has no softmax
    return inc


def pooled_ce(cand, user, cand_id, C, cand_mask=None, reject=None, col_bias=None, grad_scale=1.0):
    """cand [M, d], user [B, d] -> dict(loss [B] (0 for dead rows), loss_sum, g [B, M], duser [B, d], dcand [M, d], n_pairs,
    inc [B, M], and the absolute sums the tests build their summation bounds from: abs_duser, abs_dcand)."""
    cand, user = np.asarray(cand, dtype=np.float64), np.asarray(user, dtype=np.float64)
    B, M = user.shape[0], cand.shape[0]
    assert M == B * C
    inc = inclusion(B, C, cand_id, cand_mask, reject)
    own = np.arange(B) * C
    z = user @ cand.T
    if col_bias is not None:
        z = z + np.asarray(col_bias, dtype=np.float64).reshape(1, M)
    row_live = inc[np.arange(B), own]
    zm = np.where(inc, z, -np.inf)
    mx = np.where(row_live, zm.max(axis=1, initial=-np.inf), 0.0)
    e = np.where(inc, np.exp(np.where(inc, z, 0.0) - mx[:, None]), 0.0)
    s = e.sum(axis=1)
    lse = mx + np.log(np.where(row_live, s, 1.0))
    loss = np.where(row_live, lse - z[np.arange(B), own], 0.0)
    p = e / np.where(row_live, s, 1.0)[:, None]
    onehot = np.zeros((B, M))
    onehot[np.arange(B), own] = 1.0
    g = np.where(inc, (p - onehot) * float(grad_scale), 0.0)
    not_own = np.ones((B, M), dtype=bool)
    not_own[np.arange(B), own] = False
    return dict(loss=loss, loss_sum=float(loss.sum()), g=g, duser=g @ cand, dcand=g.T @ user, n_pairs=int((inc & not_own).sum()),
                inc=inc, abs_duser=np.abs(g) @ np.abs(cand), abs_dcand=np.abs(g).T @ np.abs(user))
