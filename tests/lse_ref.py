"""Restatement of nrms_logsumexp_dot's contract (include/nrms_hip.h, "The exact log-partition of the served softmax"),
independent of the library: the logits from given score bits (an exact fp32 fma), eligibility, the exact maximum and count,
the log-partition in float64, and `lse32`: the kernel's own arithmetic (float32 exp, the two-limb fixed-point mass added up in
integers, one float64 log) with numpy's float32 exp in place of the device's expf.  Also the shapes the GPU test runs, so that
the host test can hold the float32 restatement to its share of the tolerance on the same data."""
import numpy as np

from .softmax_sample_ref import fma32

MASS_ONE = 1 << 31                  # NRMS_LSE_MASS_ONE: the hi limb of one item at the maximum
MAX_J = 8


def logits(scores, inv_t, bias=None, bias_scale=None):
    """float32 [J, B, N]: z_j = fmaf(score, inv_t[j], c_j), c_j = bias_scale[j] * bias (one fp32 multiply), +0.0 without a bias."""
    scores = np.asarray(scores, dtype=np.float32)
    inv_t = np.asarray(inv_t, dtype=np.float32).reshape(-1)
    scale = np.ones_like(inv_t) if bias_scale is None else np.asarray(bias_scale, dtype=np.float32).reshape(-1)
    assert 1 <= inv_t.size <= MAX_J and scale.size == inv_t.size
    out = np.empty((inv_t.size,) + scores.shape, dtype=np.float32)
    for j in range(inv_t.size):
        with np.errstate(invalid="ignore", over="ignore"):
            c = np.zeros(scores.shape[1], np.float32) if bias is None else scale[j] * np.asarray(bias, dtype=np.float32)
        assert c.dtype == np.float32
        out[j] = fma32(scores, inv_t[j], c[None, :])
    return out


def eligible(z, exclude=None):
    """bool [J, B, N]: n is not in exclude[b] (ids outside [0, N) and duplicates mean nothing) and z_j(b, n) is not NaN."""
    J, B, N = z.shape
    ok = ~np.isnan(z)
    if exclude is not None:
        for b in range(B):
            ex = np.asarray(exclude[b], dtype=np.int64)
            ok[:, b, ex[(ex >= 0) & (ex < N)]] = False
    return ok


def fixed(t):
    """(hi, lo) uint64 of float32 t in [0, 1]: floor(t 2^31) and floor(frac(t 2^31) 2^32), every step in float32."""
    t = np.asarray(t, dtype=np.float32)
    x = t * np.float32(2.0 ** 31)
    xi = np.trunc(x)
    lo = (x - xi) * np.float32(2.0 ** 32)
    assert x.dtype == np.float32 and lo.dtype == np.float32
    return xi.astype(np.uint64), lo.astype(np.uint64)


def reference(scores, inv_t, bias=None, bias_scale=None, exclude=None):
    """dict of [B, J] arrays: zmax float32, n_eligible int32, lse64 float64, lse32 float32, and mass uint64 [B, J, 2]."""
    z = logits(scores, inv_t, bias, bias_scale)
    ok = eligible(z, exclude)
    J, B, N = z.shape
    zmax = np.full((B, J), -np.inf, dtype=np.float32)
    n_el = np.zeros((B, J), dtype=np.int32)
    lse64 = np.full((B, J), -np.inf, dtype=np.float64)
    lse32 = np.full((B, J), -np.inf, dtype=np.float32)
    mass = np.zeros((B, J, 2), dtype=np.uint64)
    for j in range(J):
        for b in range(B):
            v = z[j, b, ok[j, b]]
            n_el[b, j] = v.size
            if not v.size:
                continue
            m = v.max() + np.float32(0.0)                     # -0.0 -> +0.0
            zmax[b, j] = m
            if np.isinf(m):
                lse64[b, j] = lse32[b, j] = m
                continue
            with np.errstate(under="ignore"):
                lse64[b, j] = np.float64(m) + np.log(np.exp(v.astype(np.float64) - np.float64(m)).sum())
                t = np.minimum(np.exp(v - m), np.float32(1.0))
            assert t.dtype == np.float32
            hi, lo = fixed(t)
            mass[b, j] = (hi.sum(dtype=np.uint64), lo.sum(dtype=np.uint64))
            lse32[b, j] = np.float32(np.float64(m) + np.log(float(int(mass[b, j, 0])) * 2.0 ** -31 + float(int(mass[b, j, 1])) * 2.0 ** -63))
    return {"zmax": zmax, "n_eligible": n_el, "lse64": lse64, "lse32": lse32, "mass": mass, "z": z, "ok": ok}


def bar(lse32, lse64):
    """The tolerance of one case, elementwise [B, J]: 4 x the float32 restatement's own largest error on the case's data, and
    never below 2 fp32 ulps of |lse| (the rounding of the output).  Infinite entries are compared exactly, not through this."""
    fin = np.isfinite(lse64)
    with np.errstate(invalid="ignore"):
        own = float(np.abs(lse32.astype(np.float64) - lse64)[fin].max()) if fin.any() else 0.0
    floor = 2.0 * np.spacing(np.abs(np.where(fin, lse64, 1.0)).astype(np.float32)).astype(np.float64)
    return np.maximum(4.0 * own, floor), own


# ---- the shapes of tests/test_hip_lse.py ----------------------------------------------------------------------------------------
# (B, N, d, J, n_exclude, with a prior): N over the 64-item wave step, the 512-item block step and several slices; d over both
# forms of the chain, the 32-block and the groups of 8 of the remainder; n_exclude 65 is past the list length staged in LDS.
CASES = [
    (1, 1, 1, 1, 0, False), (1, 63, 7, 3, 1, True), (31, 64, 8, 1, 0, False), (32, 65, 31, 8, 50, True),
    (33, 511, 32, 3, 1, False), (65, 512, 33, 1, 65, True), (1, 513, 36, 8, 50, False), (33, 2049, 300, 3, 50, True),
    (65, 5003, 301, 8, 65, True), (32, 5003, 300, 1, 0, False), (31, 2049, 36, 8, 1, True), (5, 0, 8, 3, 0, False),
]
INV_T = np.array([1.0, 0.0, 20.0, 0.37, 2.5, 6.5, 0.05, 1.0], dtype=np.float32)
SCALE = np.array([1.0, 0.5, 0.0, -1.0, 2.0, 0.25, 1.0, 0.0], dtype=np.float32)


def case_data(case):
    """(user [B, d], items [N, d], bias [N] or None, exclude [B, n_ex] or None, inv_t [J], scale [J] or None) of one case: real
    valued rows, a few NaN rows and priors, exclude lists with id -1, N, 0 and a duplicate."""
    B, N, d, J, n_ex, prior = case
    rng = np.random.default_rng(1000 * N + 10 * d + B)
    user = rng.standard_normal((B, d)).astype(np.float32)
    items = (rng.standard_normal((N, d)) * (1.5 / np.sqrt(d))).astype(np.float32)
    if N > 8:
        items[rng.choice(N, size=max(1, N // 97), replace=False)] = np.nan
    bias = None
    if prior:
        bias = rng.standard_normal(N).astype(np.float32)
        if N > 8:
            bias[rng.choice(N, size=2, replace=False)] = np.nan
            bias[rng.integers(N)] = -np.inf
    ex = None
    if n_ex:
        ex = rng.integers(0, max(N, 1), size=(B, n_ex)).astype(np.int64)
        if n_ex > 4:
            ex[:, 0], ex[:, 1], ex[:, 2], ex[:, 3] = -1, N, 0, ex[:, 4]
    return user, items, bias, ex, INV_T[:J].copy(), (SCALE[:J].copy() if prior else None)


def host_scores(user, items):
    """float32 [B, N]: the float64 product rounded once (the host's stand-in for the chain's bits)."""
    with np.errstate(invalid="ignore"):
        return (user.astype(np.float64) @ items.astype(np.float64).T).astype(np.float32).reshape(user.shape[0], items.shape[0])
