"""The kernels every model's step ends in, one by one through the C ABI against numpy float64 (csrc/pool.hip, csrc/embed.hip):
click_fwd / click_indexed / click_bwd, ce_loss, adam<GUARD> / grad_guard, sanitize_ids.  None of them takes a workspace, so
neither the extent suite nor the guard-band suite reaches them; whole-model parity reaches them only at B <= a few dozen, C = 4
or 5, d = 60 or 300.

Bounds.  A sum of n fp32 products in any order: (n + 8) 2^-24 sum |terms|, per output element, in float64.  One product:
relative 2^-23.  Cross-entropy: no invented tolerance -- torch.nn.functional.cross_entropy(reduction="sum") and its gradient run
in fp32 on the CPU on the same inputs, their error against float64 is measured, and the kernel is allowed 4x that plus one fp32
ulp of the reference value (the kernel sums C in fp32 runs of 16 slots added up in double, and B in a 256-leaf tree, an order
torch does not share; 4x covers reordering and nothing more).  Torch's error is taken as its largest over the tensor: the error
of single elements or of a row of two is zero too often to measure anything.  Adam: oracle.adam_step at the bars of tests/test_hip_parity.py::test_adam_step_kernel_alone.
Every test prints the largest error beside its bound (docs/EXPERIMENTS.md records them).

Found by these tests and fixed with them (csrc/pool.hip; figures in docs/EXPERIMENTS.md): ce_loss_kernel formed mx + log(sum)
before it subtracted s[0], so log(sum) was rounded to an ulp of the row maximum -- a row masked in every slot (all -1e9, ulp 64)
contributed 0 instead of log(C); its serial fp32 sum over C and the device logf missed the tolerance above at C = 300 (now fp32
runs of 16 added up in double, log and reciprocal in double, rounded once per row); adam_kernel<true> and adam_kernel<false> were contracted to fma differently and disagreed in the
last bit on finite gradients (now one shared update with every rounding spelt out)."""
import ctypes as C

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import _lib

pytestmark = pytest.mark.gpu

U24, U23 = 2.0 ** -24, 2.0 ** -23
EINVAL = _lib.NRMS_EINVAL
NEG = np.float32(-1e9)


def lib():
    return _lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def poisoned(*shape):
    """fp32 NaNs (0xFFFFFFFF): a kernel that accumulates into its output, or skips an element, shows."""
    return torch.full(shape, -1, dtype=torch.int32, device="cuda").view(torch.float32)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


# ---- click scores ------------------------------------------------------------------------------------------------------------------
MASKS = ["null", "random", "user_masked", "slot0"]


def make_mask(kind, B, Cn, rng):
    if kind == "null":
        return None
    m = np.ones((B, Cn), dtype=np.uint8)
    if kind == "random":
        m = (rng.random((B, Cn)) < 0.6).astype(np.uint8)
    elif kind == "user_masked":
        m[B // 2] = 0
    else:
        m[:, 0] = 0
    return m


def click_fwd(cand, user, mask, out=None):
    B, Cn, d = cand.shape
    out = poisoned(B, Cn) if out is None else out
    rc = lib().nrms_click_score_fwd(B, Cn, d, _lib.ptr(cand), _lib.ptr(user), _lib.ptr(mask), _lib.ptr(out), _stream())
    _lib.check(rc, "nrms_click_score_fwd")
    return out


def click_indexed(vec, index, user, mask, B, Cn):
    out = poisoned(B, Cn)
    rc = lib().nrms_click_score_indexed(B, Cn, vec.shape[1], _lib.ptr(vec), vec.shape[0], _lib.ptr(index), _lib.ptr(user), _lib.ptr(mask),
                                        _lib.ptr(out), _stream())
    _lib.check(rc, "nrms_click_score_indexed")
    return out


@pytest.mark.parametrize("B,Cn", [(1, 1), (3, 5), (7, 300), (257, 3)])
@pytest.mark.parametrize("d", [1, 4, 63, 64, 65, 300, 1024])
def test_click_scores_forward_indexed_and_backward(d, B, Cn):
    rng = np.random.default_rng(1000 * d + B)
    cand = rng.standard_normal((B, Cn, d)).astype(np.float32)
    user = rng.standard_normal((B, d)).astype(np.float32)
    # the indexed form: the same candidate vectors as rows of a shuffled table with three rows nobody names
    n_vec = B * Cn + 3
    index = rng.permutation(n_vec)[:B * Cn].astype(np.int32)
    table = rng.standard_normal((n_vec, d)).astype(np.float32)
    table[index] = cand.reshape(B * Cn, d)
    c64, u64 = cand.astype(np.float64), user.astype(np.float64)
    terms = c64 * u64[:, None, :]
    ref, bound = terms.sum(-1), (d + 8) * U24 * np.abs(terms).sum(-1)
    cand_d, user_d, table_d, index_d = dev(cand), dev(user), dev(table), dev(index)
    worst = dict(fwd=0.0, dcand=0.0, duser=0.0)
    for kind in MASKS:
        mask = make_mask(kind, B, Cn, rng)
        live = np.ones((B, Cn), dtype=bool) if mask is None else mask != 0
        mask_d = None if mask is None else dev(mask)
        got_t = click_fwd(cand_d, user_d, mask_d)
        got = host(got_t)
        assert np.isfinite(got).all(), kind
        err = np.abs(got - ref)
        assert (err[live] <= bound[live]).all(), (kind, float((err - bound)[live].max()))
        worst["fwd"] = max(worst["fwd"], float((err[live] / bound[live]).max(initial=0.0)))
        assert (bits(got[~live]) == bits(NEG)).all(), kind                       # masked slots: exactly -1e9f
        idx = host(click_indexed(table_d, index_d, user_d, mask_d, B, Cn))
        assert np.array_equal(bits(idx), bits(got)), kind                         # bit-equal to the materialised candidates
        # backward: dscores at masked slots is large and must not be read
        ds = (rng.standard_normal((B, Cn)) * 0.1).astype(np.float32)
        ds_in = np.where(live, ds, np.float32(1e30))
        dcand_o, duser_o = poisoned(B, Cn, d), poisoned(B, d)
        rc = lib().nrms_click_score_bwd(B, Cn, d, _lib.ptr(cand_d), _lib.ptr(user_d), _lib.ptr(mask_d), _lib.ptr(dev(ds_in)),
                                        _lib.ptr(dcand_o), _lib.ptr(duser_o), _stream())
        _lib.check(rc, "nrms_click_score_bwd")
        dc, du = host(dcand_o), host(duser_o)
        g64 = np.where(live, ds, 0).astype(np.float64)
        dc_ref = g64[:, :, None] * u64[:, None, :]
        assert (np.abs(dc - dc_ref) <= U23 * np.abs(dc_ref)).all(), kind            # one product each (poison overwritten)
        assert (dc[~live] == 0).all(), kind                                       # masked slots: exactly zero rows
        du_terms = g64[:, :, None] * c64
        du_err, du_bound = np.abs(du - du_terms.sum(1)), (Cn + 8) * U24 * np.abs(du_terms).sum(1)
        assert (du_err <= du_bound).all(), (kind, float((du_err - du_bound).max()))
        if kind == "user_masked":
            assert (du[B // 2] == 0).all()                                        # a fully masked user: no gradient at all
        nz = dc_ref != 0
        worst["dcand"] = max(worst["dcand"], float((np.abs(dc - dc_ref)[nz] / np.abs(dc_ref)[nz]).max(initial=0.0)) / U23)
        worst["duser"] = max(worst["duser"], float((du_err[du_bound > 0] / du_bound[du_bound > 0]).max(initial=0.0)))
    print("click d=%d B=%d C=%d: worst error / bound: scores %.3f, dcand %.3f, duser %.3f" % (d, B, Cn, worst["fwd"], worst["dcand"], worst["duser"]))
    # an index of -1 or n_vec scores NaN and leaves every other slot as it was
    base = host(click_indexed(table_d, index_d, user_d, None, B, Cn)).reshape(-1)
    bad = index.copy()
    where = sorted({0, (B * Cn) // 2, B * Cn - 1})
    for k, slot in enumerate(where):
        bad[slot] = -1 if k % 2 == 0 else n_vec
    got = host(click_indexed(table_d, dev(bad), user_d, None, B, Cn)).reshape(-1)
    assert np.isnan(got[where]).all()
    rest = np.setdiff1d(np.arange(B * Cn), where)
    assert np.array_equal(bits(got[rest]), bits(base[rest]))


def test_click_scores_of_an_empty_batch_touch_nothing():
    d, Cn = 8, 3
    cand, user = dev(np.ones((1, Cn, d), np.float32)), dev(np.ones((1, d), np.float32))
    index = dev(np.zeros(Cn, np.int32))
    out, dc, du = poisoned(1, Cn), poisoned(1, Cn, d), poisoned(1, d)
    L = lib()
    assert L.nrms_click_score_fwd(0, Cn, d, _lib.ptr(cand), _lib.ptr(user), None, _lib.ptr(out), _stream()) == 0
    assert L.nrms_click_score_indexed(0, Cn, d, _lib.ptr(cand.view(Cn, d)), Cn, _lib.ptr(index), _lib.ptr(user), None, _lib.ptr(out), _stream()) == 0
    assert L.nrms_click_score_bwd(0, Cn, d, _lib.ptr(cand), _lib.ptr(user), None, _lib.ptr(out), _lib.ptr(dc), _lib.ptr(du), _stream()) == 0
    for t in (out, dc, du):
        assert (bits(host(t)) == 0xFFFFFFFF).all()


# ---- cross-entropy -----------------------------------------------------------------------------------------------------------------
SCORE_SETS = ["n01", "n30", "equal", "some_masked", "all_but_0_masked", "all_masked", "spread_1e4"]


def make_scores(kind, B, Cn, rng):
    s = rng.standard_normal((B, Cn)).astype(np.float32)
    rows = np.arange(B) % 3 == 0                                                 # row 0 and every third row after it
    if kind == "n30":
        s = (s * np.float32(30.0)).astype(np.float32)
    elif kind == "equal":
        s[:] = np.float32(0.7310586)
    elif kind == "some_masked":
        s[np.ix_(rows, np.arange(Cn) % 2 == 1)] = NEG
    elif kind == "all_but_0_masked":
        s[np.ix_(rows, np.arange(Cn) > 0)] = NEG
    elif kind == "all_masked":
        s[rows] = NEG
    elif kind == "spread_1e4":
        s[B // 2] = rng.permutation(np.linspace(-5e3, 5e3, Cn)).astype(np.float32)
    return s


def ce_ref(s, gs):
    """float64: (sum_b logsumexp(s_b) - s_b0, (softmax - onehot0) * float64(float32(gs)))."""
    s = s.astype(np.float64)
    mx = s.max(1, keepdims=True)
    e = np.exp(s - mx)
    z = e.sum(1, keepdims=True)
    loss = float(((mx[:, 0] - s[:, 0]) + np.log(z[:, 0])).sum())
    g = e / z
    g[:, 0] -= 1.0
    return loss, g * float(np.float32(gs))


def ce_torch_fp32(s, gs):
    t = torch.from_numpy(s.copy()).requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(t, torch.zeros(len(s), dtype=torch.long), reduction="sum")
    loss.backward(torch.tensor(gs, dtype=torch.float32))
    return float(loss.detach()), t.grad.numpy()


def ce_kernel(s_d, gs, loss_cell=None, want_grad=True):
    B, Cn = s_d.shape
    loss = torch.zeros(1, dtype=torch.float32, device="cuda") if loss_cell is None else loss_cell
    ds = poisoned(B, Cn) if want_grad else None
    rc = lib().nrms_ce_loss_fwd_bwd(B, Cn, _lib.ptr(s_d), _lib.ptr(loss), _lib.ptr(ds), C.c_float(gs), _stream())
    _lib.check(rc, "nrms_ce_loss_fwd_bwd")
    return loss, ds


@pytest.mark.parametrize("Cn", [1, 2, 5, 300])
@pytest.mark.parametrize("B", [1, 2, 255, 256, 257, 1000])
def test_cross_entropy_loss_and_gradient(B, Cn):
    rng = np.random.default_rng(100 * B + Cn)
    for kind in SCORE_SETS:
        s = make_scores(kind, B, Cn, rng)
        s_d = dev(s)
        for gs in (1.0, 1.0 / B, 1.0 / 4096):
            r_loss, r_grad = ce_ref(s, gs)
            t_loss, t_grad = ce_torch_fp32(s, gs)
            loss_t, ds_t = ce_kernel(s_d, gs)
            k_loss, k_grad = float(host(loss_t)[0]), host(ds_t)
            e_t, e_k = abs(t_loss - r_loss), abs(k_loss - r_loss)
            g_t, g_k = float(np.abs(t_grad - r_grad).max()), np.abs(k_grad - r_grad)
            allow_loss = 4 * e_t + float(ulp32(r_loss))
            allow_grad = 4 * g_t + ulp32(r_grad)
            rowsum = np.abs(k_grad.astype(np.float64).sum(1))
            gs32 = float(np.float32(gs))
            print("ce B=%d C=%d %-17s gs=%.2e  loss: torch %.2e kernel %.2e allowed %.2e (ref %.6g) | grad: torch %.2e kernel %.2e "
                  "allowed %.2e | row sum %.2e of %.2e" % (B, Cn, kind, gs, e_t, e_k, allow_loss, r_loss, g_t, float(g_k.max()),
                                                           float(allow_grad.min()), float(rowsum.max()), Cn * U23 * gs32))
            assert np.isfinite(k_loss) and np.isfinite(k_grad).all()
            assert e_k <= allow_loss, (kind, gs, k_loss, r_loss, e_k, allow_loss)
            assert (g_k <= allow_grad).all(), (kind, gs, float((g_k - allow_grad).max()))
            assert (rowsum <= Cn * U23 * gs32).all(), (kind, gs, float(rowsum.max()))
            if Cn == 1:
                assert k_loss == 0.0 and not k_grad.any()
        # loss only: the same loss bits; and the cell accumulates -- two calls into one preset nonzero cell give the sum
        one, _ = ce_kernel(s_d, 1.0)
        alone, none = ce_kernel(s_d, 1.0, want_grad=False)
        assert none is None and np.array_equal(bits(host(alone)), bits(host(one))), kind
        cell = torch.full((1,), 3.25, dtype=torch.float32, device="cuda")
        ce_kernel(s_d, 1.0, loss_cell=cell)
        ce_kernel(s_d, 1.0, loss_cell=cell)
        v = np.float32(host(one)[0])
        assert host(cell)[0] == np.float32(np.float32(np.float32(3.25) + v) + v), kind


@pytest.mark.parametrize("B,Cn", [(1, 5), (257, 5), (300, 2)])
def test_cross_entropy_nan_stays_in_its_row(B, Cn):
    rng = np.random.default_rng(B)
    s = rng.standard_normal((B, Cn)).astype(np.float32)
    row = B // 2
    s[row, Cn - 1] = np.nan
    loss, ds = ce_kernel(dev(s), 1.0)
    g = host(ds)
    assert np.isnan(host(loss)[0])
    assert np.isnan(g[row]).all()
    others = np.delete(g, row, axis=0)
    assert np.isfinite(others).all()
    s[row, Cn - 1] = 0.5                                                         # rows are independent: the same bits without the NaN
    _, ds2 = ce_kernel(dev(s), 1.0)
    assert np.array_equal(bits(np.delete(host(ds2), row, axis=0)), bits(others)) and np.isfinite(host(ds2)).all()


def test_cross_entropy_of_an_empty_batch_touches_nothing():
    cell, ds = torch.full((1,), 3.25, dtype=torch.float32, device="cuda"), poisoned(1, 4)
    assert lib().nrms_ce_loss_fwd_bwd(0, 4, _lib.ptr(ds), _lib.ptr(cell), _lib.ptr(ds), C.c_float(1.0), _stream()) == 0
    assert host(cell)[0] == 3.25 and (bits(host(ds)) == 0xFFFFFFFF).all()


# ---- Adam, guarded Adam, grad_guard ------------------------------------------------------------------------------------------------
BIG = 2_097_152 + 4 + 3          # 2048 blocks x 256 threads x 4 floats, one more float4 (the capped grid's second turn) and a tail of 3
SIZES = [1, 2, 3, 4, 5, 1023, 1024, BIG]
HYPER = {"default": dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8), "other": dict(lr=3e-4, b1=0.8, b2=0.99, eps=1e-6)}


def adam_inputs(n, seed):
    rng = np.random.default_rng(seed)
    p = rng.normal(0, 0.3, n).astype(np.float32)
    g = (rng.normal(0, 1, n) * 10.0 ** rng.uniform(-9, -1, n)).astype(np.float32)
    m = (rng.normal(0, 1, n) * 1e-3).astype(np.float32)                          # nonzero moments: a step in the middle of training
    v = (rng.uniform(0.1, 1.0, n) * 1e-6).astype(np.float32)
    return p, g, m, v


def adam_call(n, p, g, m, v, step, hp, gs=1.0, counter=None, guarded=False):
    args = [C.c_size_t(n), _lib.ptr(p), _lib.ptr(g), _lib.ptr(m), _lib.ptr(v), C.c_double(hp["lr"]), C.c_double(hp["b1"]),
            C.c_double(hp["b2"]), C.c_double(hp["eps"]), int(step), C.c_float(gs)]
    if guarded:
        return lib().nrms_adam_step_guarded(*args, _lib.ptr(counter), _stream())
    return lib().nrms_adam_step(*args, _stream())


def adam_oracle(p, g, m, v, step, hp, gs=1.0):
    from oracle import nrms_oracle as orc
    p, m, v = p.copy(), m.copy(), v.copy()
    with np.errstate(all="ignore"):
        orc.adam_step(p, (g * np.float32(gs)).astype(np.float32), m, v, step, lr=hp["lr"], b1=hp["b1"], b2=hp["b2"], eps=hp["eps"])
    return p, m, v


def assert_adam_close(got, want, sel, what):
    """The bars of test_adam_step_kernel_alone: 1.5e-7 absolute on parameters of scale 0.3, rtol 2e-6 / 4e-6 on m / v."""
    (gp, gm, gv), (wp, wm, wv) = got, want
    with np.errstate(all="ignore"):
        errs = (float(np.abs(gp - wp)[sel].max(initial=0.0)), float((np.abs(gm - wm) / np.abs(wm))[sel].max(initial=0.0)),
                float((np.abs(gv - wv) / np.abs(wv))[sel].max(initial=0.0)))
    assert errs[0] <= 1.5e-7, (what, errs)
    np.testing.assert_allclose(gm[sel], wm[sel], rtol=2e-6, atol=2e-7 * float(np.abs(wm[sel]).max(initial=0.0)), err_msg=what)
    np.testing.assert_allclose(gv[sel], wv[sel], rtol=4e-6, atol=2e-7 * float(np.abs(wv[sel]).max(initial=0.0)), err_msg=what)
    return errs


@pytest.mark.parametrize("n,hyper", [(n, "default") for n in SIZES] + [(5, "other"), (BIG, "other")])
def test_adam_step_element_by_element(n, hyper):
    hp = HYPER[hyper]
    p, g, m, v = adam_inputs(n, seed=n)
    everything = np.ones(n, dtype=bool)
    for step in (1, 2, 10_000):
        for gs in ((1.0, 0.25) if step == 2 else (1.0,)):                         # grad_scale: the 1 / world_size of data parallel
            want = adam_oracle(p, g, m, v, step, hp, gs)
            dp, dg, dm, dv = dev(p), dev(g), dev(m), dev(v)
            assert adam_call(n, dp, dg, dm, dv, step, hp, gs) == 0
            got = (host(dp), host(dm), host(dv))
            errs = assert_adam_close(got, want, everything, "n=%d step=%d gs=%g" % (n, step, gs))
            assert np.array_equal(host(dg), g)
            # guarded == unguarded, bit for bit, on finite gradients; the counter stays where it was
            gp, gm, gv, cnt = dev(p), dev(m), dev(v), torch.full((1,), 7, dtype=torch.int32, device="cuda")
            assert adam_call(n, gp, dg, gm, gv, step, hp, gs, counter=cnt, guarded=True) == 0
            assert all(np.array_equal(bits(host(a)), bits(b)) for a, b in zip((gp, gm, gv), got)) and int(cnt.item()) == 7
        print("adam n=%d %s step %d: max |dp| %.2e (bar 1.5e-7), rel m %.2e (2e-6), rel v %.2e (4e-6)" % ((n, hyper, step) + errs))


def plant_positions(n):
    """The vector body of the first stride, the second stride of the capped grid, and each position of the scalar tail."""
    n4 = n // 4
    want = [0, 5, 1021, 4 * 524_288 + 2] + list(range(4 * n4, n))
    return sorted({i for i in want if i < n})


@pytest.mark.parametrize("kind", ["nonfinite", "overflow"])
@pytest.mark.parametrize("n", SIZES)
def test_guarded_adam_skips_nonfinite_gradients_and_counts_them(n, kind):
    hp = HYPER["default"]
    p, g, m, v = adam_inputs(n, seed=n + 1)
    pos = plant_positions(n)
    if kind == "nonfinite":
        gs = 1.0
        g[pos] = np.resize(np.array([np.inf, -np.inf, np.nan], dtype=np.float32), len(pos))
    else:
        # finite gradients whose product with grad_scale = 2^100 overflows; the others are small enough to stay finite
        gs = 2.0 ** 100
        rng = np.random.default_rng(n)
        g = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-5, -1, n) * 2.0 ** -100).astype(np.float32)
        g[pos] = np.resize(np.array([1e10, -1e10], dtype=np.float32), len(pos))
        assert np.isfinite(g).all()
    planted = np.zeros(n, dtype=bool)
    planted[pos] = True
    clean = np.where(planted, np.float32(0), g)
    dp, dg, dm, dv = dev(p), dev(g), dev(m), dev(v)
    cnt = torch.full((1,), 11, dtype=torch.int32, device="cuda")
    state = (p, m, v)
    for call, step in enumerate((3, 4), start=1):
        want = adam_oracle(*state[:1], clean, *state[1:], step, hp, gs)
        assert adam_call(n, dp, dg, dm, dv, step, hp, gs, counter=cnt, guarded=True) == 0
        got = (host(dp), host(dm), host(dv))
        for a, b in zip(got, (p, m, v)):
            assert np.array_equal(bits(a[planted]), bits(b[planted]))              # p, m, v keep their bits
        assert all(np.isfinite(a).all() for a in got)
        assert_adam_close(got, want, ~planted, "n=%d %s call %d" % (n, kind, call))
        assert int(cnt.item()) == 11 + call * len(pos)                            # exact, and accumulated over two calls
        state = tuple(np.where(planted, b, w) for b, w in zip((p, m, v), want))   # the next call continues from the oracle's state
        dp, dm, dv = dev(state[0]), dev(state[1]), dev(state[2])


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", SIZES)
def test_grad_guard_zeroes_nonfinite_elements_and_counts_them(n, offset):
    """offset 1: a view one float into the allocation -- not 16-byte aligned, the kernel's scalar path."""
    _, g, _, _ = adam_inputs(n, seed=n + 2)
    g[g == 0] = np.float32(1e-3)
    pos = plant_positions(n)
    g[pos] = np.resize(np.array([np.inf, -np.inf, np.nan], dtype=np.float32), len(pos))
    buf = poisoned(n + 2)
    view = buf[offset:offset + n]
    view.copy_(torch.from_numpy(g))
    assert (view.data_ptr() % 16 == 0) == (offset == 0)
    cnt = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    for call in (1, 2):
        assert lib().nrms_grad_guard(C.c_size_t(n), _lib.ptr(view), _lib.ptr(cnt), _stream()) == 0
        got = host(buf)
        out = got[offset:offset + n]
        assert (bits(out[pos]) == 0).all()                                        # +0.0
        keep = np.setdiff1d(np.arange(n), pos)
        assert np.array_equal(bits(out[keep]), bits(g[keep]))
        assert (bits(got[:offset]) == 0xFFFFFFFF).all() and (bits(got[offset + n:]) == 0xFFFFFFFF).all()
        assert int(cnt.item()) == 5 + len(pos)                                    # the second call finds nothing more


def test_adam_refuses_a_misaligned_view_and_an_empty_one_is_a_no_op():
    hp = HYPER["default"]
    n = 1024
    p, g, m, v = adam_inputs(n + 1, seed=9)
    for which in range(4):
        full = [dev(a) for a in (p, g, m, v)]
        views = [t[1:] if k == which else t[:n] for k, t in enumerate(full)]
        cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        assert adam_call(n, *views, 1, hp) == EINVAL
        assert b"aligned" in lib().nrms_last_error()
        assert adam_call(n, *views, 1, hp, counter=cnt, guarded=True) == EINVAL
        assert all(np.array_equal(bits(host(t)), bits(a)) for t, a in zip(full, (p, g, m, v))) and int(cnt.item()) == 0
    full = [dev(a) for a in (p, g, m, v)]
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert adam_call(0, *full, 1, hp) == 0 and adam_call(0, *full, 1, hp, counter=cnt, guarded=True) == 0
    assert lib().nrms_grad_guard(C.c_size_t(0), _lib.ptr(full[1]), _lib.ptr(cnt), _stream()) == 0
    assert all(np.array_equal(bits(host(t)), bits(a)) for t, a in zip(full, (p, g, m, v))) and int(cnt.item()) == 0


# ---- nrms_sanitize_ids / _i32 ------------------------------------------------------------------------------------------------------
VOCAB = 1000
SPECIAL64 = [-1, VOCAB, VOCAB - 1, 0, 2 ** 31, 2 ** 40 + 3, -2 ** 63]          # 2^40 + 3 is in range once truncated to 32 bits
SPECIAL32 = [-1, VOCAB, VOCAB - 1, 0, -2 ** 31, 2 ** 31 - 1]


@pytest.mark.parametrize("width", [64, 32])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1023, 1024, 1025, 7 * 1024 + 5])
def test_sanitize_ids(n, width):
    rng = np.random.default_rng(n + width)
    special = SPECIAL64 if width == 64 else SPECIAL32
    src = rng.integers(0, VOCAB, size=n).astype(np.int64)
    where = rng.permutation(n)[:min(n, 3 * len(special))]
    src[where] = np.resize(np.array(special, dtype=np.int64), len(where))
    if n > 1:
        src[n - 1] = special[0]                                                   # the last element of the last block
    src = src.astype(np.int64 if width == 64 else np.int32)
    ok = (src >= 0) & (src < VOCAB)
    want = np.where(ok, src, 0).astype(np.int64)
    n_bad_want = int((~ok).sum())
    fn = lib().nrms_sanitize_ids if width == 64 else lib().nrms_sanitize_ids_i32
    src_d = dev(src)
    dst = torch.full((n + 1,), -7, dtype=torch.int64, device="cuda")
    cnt = torch.full((1,), 3, dtype=torch.int32, device="cuda")
    for call in (1, 2):
        assert fn(_lib.ptr(src_d), _lib.ptr(dst), n, VOCAB, _lib.ptr(cnt), _stream()) == 0
        out = host(dst)
        assert np.array_equal(out[:n], want) and out[n] == -7
        assert int(cnt.item()) == 3 + call * n_bad_want                            # accumulates over two calls
    assert np.array_equal(host(src_d), src)
    if width == 64:                                                               # dst may alias src
        cnt.zero_()
        assert fn(_lib.ptr(src_d), _lib.ptr(src_d), n, VOCAB, _lib.ptr(cnt), _stream()) == 0
        assert np.array_equal(host(src_d), want) and int(cnt.item()) == n_bad_want
    assert fn(_lib.ptr(src_d), _lib.ptr(dst), 0, VOCAB, _lib.ptr(cnt), _stream()) == 0      # n = 0: nothing happens
