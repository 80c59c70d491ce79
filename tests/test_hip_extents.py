"""The encoder chain at the upper ends of the domain validate_desc (csrc/capi.hip) accepts, against the float64 oracle.

Every other parity test draws d <= 316 and a handful of users; the C ABI admits n_seq * seq_len < 2^31 rows and d_model <= 1024.
Two pieces of index arithmetic were only right inside the tested range, and both gave wrong numbers silently:

  1. the d(ctx) epilogue of the additive-attention backward (csrc/gemm.h, E_DCTX) found a row's sequence by a float
     reciprocal, (long)((row + 0.5f) * (1.0f / S)).  Mirrored in numpy float32 (test_float_reciprocal_first_wrong_rows) its
     first wrong row is 4 397 273 at S = 63, 5 093 099 at S = 30, 5 767 178 at S = 11; from 2^23 on about every second
     sequence boundary is wrong.  A weight gradient sums millions of rows and hides one misplaced row: only a per-row output
     (the user encoder's dx) shows it.  The kernel now uses csrc/rowdiv.h, exact below 2^31.
  2. the 32 x 32 attention tiles (csrc/attention.hip, PrefetchQKV) kept a global offset in 15 bits; it overflows from
     d_model = 704 at S = 32, d_k = 32 and for d_model = 768 with 24 heads at S >= 30.  The launcher now sends those shapes to
     the unpacked form.

Tolerances are the project's stated ones (tests/test_hip_parity.py TOL: fp32 outputs 1e-5, gradients rtol 1e-3 + atol 2e-6;
the bf16x3 row adds 2e-5 of a tensor's scale), W_K.bias as tests/test_hip_v1.py bounds it (an analytically zero sum: the scale
of d(b_Q)); the fp16 case uses the fp16 bars of tests/test_hip_fuzz.py / test_hip_fp16.py (vectors 1.5e-3, gradients 8e-3 of a
tensor's scale + 1e-4 of the largest).  A misplaced row or a wrong address is off by the size of the data, orders of magnitude
beyond any of them.

The many-row inputs are i.i.d. per sequence (a neighbour's dout must be visible) with a NON-ZERO MEAN: a weight gradient over
9 M rows of zero-mean data is a cancelling sum of size sqrt(M) whose fp32 summation noise (~ eps M / sqrt(partials)) would be
measured against rtol * |ref| of its smallest elements; with a mean the sums are coherent and the relative bound means what it
says.

Memory: the largest many-row user-encoder case (S = 30, 300 000 sequences = 9.0 M rows of width 8) allocates on the device
x 288 MB + qkv 864 MB + ctx 288 MB + t 144 MB + w 36 MB, the backward workspace d(ctx) 288 MB + d(qkv) 864 MB + ds 36 MB
(+ partials), dx 288 MB: 3.1 GB; the test asserts its measured peak stays under 4 GB.  The fp16 case is the exception: the
fp16 activations have fixed 320 / 224-column pitches (include/nrms_hip.h) whatever d_model is, so 300 000 titles of 30 words
take 17 GB of activations and a 34 GB backward workspace (nrms_encoder_bwd_workspace_bytes); it prints its measured peak."""
import os
import shutil
import subprocess
import time

import numpy as np
import pytest
import torch

from pytorch_news_recommender_amd import synth

from tests.test_hip_parity import MODES, TOL, assert_grad_close

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (S, first row the float reciprocal got wrong): the table of the defect, restated by test_float_reciprocal_first_wrong_rows
FIRST_WRONG = {63: 4397273, 30: 5093099, 11: 5767178}
MANY = [(30, 300000), (63, 140000), (11, 800000)]          # each passes 2^23 rows and contains its first wrong row


# ---- row -> sequence: CPU only --------------------------------------------------------------------------------------------
def row_div_params(S):
    """csrc/rowdiv.h make_row_div, in Python integers."""
    l = 0
    while (1 << l) < S:
        l += 1
    shift = 31 + l
    return ((1 << shift) + S - 1) // S, shift


def row_div(rows, mul, shift):
    """csrc/rowdiv.h row_div with its types: a uint32 row times a uint32 multiplier as uint64, shifted right."""
    assert mul < 2 ** 32
    return (rows.astype(np.uint32).astype(np.uint64) * np.uint64(mul)) >> np.uint64(shift)


def boundary_rows(S):
    """Sequence boundaries k S - 1, k S below 2^31: every one below 2^24 (that includes every row of FIRST_WRONG and the
    range from 2^23 on where the float form failed densely), 2^18 evenly spread k beyond, and the last 4096 below 2^31."""
    kmax = (2 ** 31 - 1) // S
    dense = np.arange(1, min(kmax, 2 ** 24 // S + 1) + 1, dtype=np.int64)
    spread = np.linspace(1, kmax, num=2 ** 18, dtype=np.int64)
    last = np.arange(max(1, kmax - 4095), kmax + 1, dtype=np.int64)
    k = np.unique(np.concatenate([dense, spread, last]))
    rows = np.concatenate([k * S - 1, k * S, [0, 2 ** 31 - 1]])
    return rows[rows < 2 ** 31]


def test_row_to_sequence_is_exact_below_2_31():
    for S in range(1, 65):
        mul, shift = row_div_params(S)
        rows = boundary_rows(S)
        got = row_div(rows, mul, shift)
        bad = np.nonzero(got != (rows // S).astype(np.uint64))[0]
        assert bad.size == 0, "S=%d: row %d -> %d, not %d" % (S, rows[bad[0]], got[bad[0]], rows[bad[0]] // S)
    for S, row in FIRST_WRONG.items():
        assert row in set(boundary_rows(S).tolist())


def test_float_reciprocal_first_wrong_rows():
    """The expression the kernel used until now, with its types: the table of the defect (and why the sizes under test until
    now, at most 844 800 rows, never met it)."""
    first = {}
    for S in range(1, 65):
        rows = np.arange(2 ** 24, dtype=np.int64)
        inv = np.float32(1.0) / np.float32(S)
        seq = ((rows.astype(np.float32) + np.float32(0.5)) * inv).astype(np.int64)
        bad = np.nonzero(seq != rows // S)[0]
        first[S] = int(bad[0]) if bad.size else None
    assert {S: first[S] for S in FIRST_WRONG} == FIRST_WRONG
    wrong = [r for r in first.values() if r is not None]
    assert min(wrong) == FIRST_WRONG[63]
    assert max(wrong) < 2 ** 23 + 1024


def test_rowdiv_header_on_the_host(tmp_path):
    """csrc/rowdiv.h itself (the kernel's own code, compiled for the host): every sequence boundary below 2^27 for every
    S in 1..64, a stride beyond, the last million rows below 2^31, and the multipliers the Python mirror above uses."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    src = tmp_path / "rowdiv_check.cc"
    src.write_text(
        '#include "rowdiv.h"\n#include <stdio.h>\n'
        "int main() {\n"
        "    unsigned long long bad = 0, n = 0, first = 0; unsigned first_S = 0;\n"
        "    for (uint32_t S = 1; S <= 64; ++S) {\n"
        "        const nrms::RowDiv r = nrms::make_row_div(S);\n"
        '        printf("%u %u %u\\n", S, r.mul, r.shift);\n'
        "        auto chk = [&](uint64_t row) {\n"
        "            if (row >= (1ull << 31)) return;\n"
        "            ++n;\n"
        "            if (nrms::row_div((uint32_t)row, r) != row / S && !bad++) { first = row; first_S = S; }\n"
        "        };\n"
        "        for (uint64_t k = 1; k * S < (1ull << 27); ++k) { chk(k * S - 1); chk(k * S); }\n"
        "        for (uint64_t k = (1ull << 27) / S; k * S < (1ull << 31); k += 509) { chk(k * S - 1); chk(k * S); }\n"
        "        for (uint64_t row = (1ull << 31) - 1000000; row < (1ull << 31); ++row) chk(row);\n"
        "    }\n"
        '    printf("bad %llu of %llu first %llu S %u\\n", bad, n, first, first_S);\n'
        "    return 0;\n}\n")
    exe = tmp_path / "rowdiv_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I",
                    os.path.join(ROOT, "pytorch_news_recommender_amd", "csrc"), str(src), "-o", str(exe)],
                   check=True, capture_output=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    for line in out[:-1]:
        S, mul, shift = (int(x) for x in line.split())
        assert (mul, shift) == row_div_params(S), line
    assert out[-1].startswith("bad 0 of "), out[-1]


# ---- engine-level plumbing ----------------------------------------------------------------------------------------------
def make_engine(V, d, h, q, mode, wo=False, seed=3, table_mean=0.0):
    """An NRMSEngine on its own flat parameter buffer (v0 names; wo: with the output projection W_O)."""
    from pytorch_news_recommender_amd.engine import FlatLayout, ModelDims, NRMSEngine
    shape = synth.Shape(n_words=V, word_embed_size=d, num_attention_heads=h, query_vector_dim=q)
    params = synth.make_params(shape, seed=seed, with_output_proj=wo)
    if table_mean:
        params["news_encoder.word_embedding.0.weight"][1:] += np.float32(table_mean)
    dims = ModelDims(V, d, h, q, output_proj=wo)
    layout = FlatLayout(dims)
    flat = torch.zeros(layout.total, dtype=torch.float32, device="cuda")
    for n, v in params.items():
        layout.view(flat, n).copy_(torch.from_numpy(v))
    eng = NRMSEngine(dims, "cuda", precision=mode, layout=layout)
    return eng, flat, layout, params


def encode_titles_backward(eng, flat, gflat, ids, dout, mask=None, mask_mode=0):
    """Backward of eng.encode_titles(save=True) alone (NRMSEngine.backward runs it inside the whole model's)."""
    import ctypes as C
    from pytorch_news_recommender_amd import _lib
    from pytorch_news_recommender_amd.engine import _stream
    N, L = ids.shape
    eng.loss_scale = -float(eng.loss_scale_backoff)
    desc = eng._desc("news_encoder", N, L, mask_mode=mask_mode if mask is not None else 0, training=True)
    ws = eng._bwd_workspace(desc)
    acts = eng._acts("news", N * L, True, gather=True, desc=desc)
    if desc.precision == _lib.NRMS_PRECISION_FP16:
        desc.flags |= _lib.NRMS_FLAG_FWD_SCRATCH_KEPT
    w, g = eng._weights(flat, "news_encoder"), eng._grads(gflat, "news_encoder")
    rc = eng.lib.nrms_encoder_bwd(C.byref(desc), C.byref(w), _lib.ptr(ids), None, _lib.ptr(mask), C.byref(acts),
                                  _lib.ptr(dout.contiguous()), C.byref(g), None, _lib.ptr(ws), C.c_size_t(ws.numel() * 4),
                                  _stream())
    _lib.check(rc, "nrms_encoder_bwd(news)")
    return desc


def reference(params, enc, heads, x, dout, mask=None, mask_mode=0, slice_seqs=4096):
    """float64 oracle of one encoder pass, forward and backward, in slices of sequences (bounded host memory; the parameter
    gradients accumulate over the slices).  x: [n, S, d] float32 (user encoder) or [n, L] int64 ids (news encoder).
    -> out [n, d], dx [n, S, d] (None for ids), {name: gradient} for the encoder's tensors, all float64."""
    from oracle import nrms_oracle as orc
    keys = [k for k in params if k.startswith(enc) or (enc == "news_encoder" and "word_embedding" in k)]
    p = orc.to_torch({k: params[k] for k in keys}, dtype=torch.float64, requires_grad=True)
    n = x.shape[0]
    user = enc == "user_encoder"
    out = np.empty((n, dout.shape[1]), dtype=np.float64)
    dx = np.empty(x.shape, dtype=np.float64) if user else None
    for s0 in range(0, n, slice_seqs):
        s1 = min(n, s0 + slice_seqs)
        m = None if mask is None else torch.from_numpy(mask[s0:s1])
        if user:
            xt = torch.from_numpy(x[s0:s1]).double().requires_grad_(True)
            o = orc.user_encoder(p, xt, heads, mask=m, mask_mode=mask_mode)
        else:
            o = orc.news_encoder(p, torch.from_numpy(x[s0:s1]), heads, mask=m, mask_mode=mask_mode)
        (o * torch.from_numpy(dout[s0:s1]).double()).sum().backward()
        out[s0:s1] = o.detach().numpy()
        if user:
            dx[s0:s1] = xt.grad.numpy()
    return out, dx, {k: t.grad.numpy() for k, t in p.items() if t.grad is not None}


_REF_CACHE = {}


def cached_reference(key, *args, **kw):
    """The last reference only: the two precision modes of one case share it, a new case drops it (host memory)."""
    if key not in _REF_CACHE:
        _REF_CACHE.clear()
        _REF_CACHE[key] = reference(*args, **kw)
    return _REF_CACHE[key]


def first_bad_row(got, ref, mode):
    """(first row of [rows, d] outside assert_grad_close's bound or None, number of such rows, max |diff|)."""
    t = TOL[mode]
    bound = t["g_rtol"] * np.abs(ref) + t["g_atol"] + t["g_scale"] * float(np.abs(ref).max())
    diff = np.abs(got - ref)
    rows = np.nonzero((diff > bound).any(axis=1))[0]
    return (int(rows[0]) if rows.size else None), int(rows.size), float(diff.max())


def check_param_grads(layout, gflat, r_grads, mode, what):
    worst = {}
    for name, ref in r_grads.items():
        got = layout.view(gflat, name).cpu().numpy()
        worst[name] = float(np.abs(got - ref).max() / max(float(np.abs(ref).max()), 1e-30))
        if name.endswith("W_K.bias"):
            # exactly zero without a mask (softmax rows sum to one): a cancelling sum of the terms of d(b_Q), bounded by that
            # tensor's scale (tests/test_hip_v1.py::test_masked_primitives_forward_backward)
            qb = r_grads[name.replace("W_K.bias", "W_Q.bias")]
            t = TOL[mode]
            err = float(np.abs(got - ref).max())
            assert err <= t["g_atol"] + (t["g_rtol"] + t["g_scale"]) * float(np.abs(qb).max()), (what, name, err)
            continue
        assert_grad_close(got, ref, mode, "%s %s" % (what, name))
    return worst


# ---- 1. many rows, narrow model -------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S,n_seq", MANY)
def test_many_rows_user_encoder(S, n_seq, mode):
    """One user-encoder pass (vocab == 0) over more than 2^23 rows of width 8 on the GEMM -> attention -> additive chain: out,
    EVERY row of dx and the weight gradients.  Before csrc/rowdiv.h the first wrong row of dx was FIRST_WRONG[S]."""
    d, h, q = 8, 2, 4
    assert n_seq * S > 2 ** 23 and FIRST_WRONG[S] < n_seq * S
    eng, flat, layout, params = make_engine(4, d, h, q, mode)
    eng.fused_user_encoder = False                 # the chain (E_DCTX); the one-kernel form has a test of its own below
    rng = np.random.default_rng(1000 + S)
    x = rng.normal(0.2, 0.5, size=(n_seq, S, d)).astype(np.float32)
    dout = rng.normal(0.3, 1.0, size=(n_seq, d)).astype(np.float32)
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    xd, dd = torch.from_numpy(x).cuda(), torch.from_numpy(dout).cuda()
    out = eng.encode_users(flat, xd, save=True)
    gflat = torch.zeros_like(flat)
    dx = eng.encode_users_backward(flat, gflat, xd, dd)
    torch.cuda.synchronize()
    t_gpu = time.time() - t0
    peak = torch.cuda.max_memory_allocated()
    out, dx = out.cpu().numpy(), dx.cpu().numpy().reshape(n_seq * S, d)
    del xd, dd
    t0 = time.time()
    r_out, r_dx, r_grads = cached_reference(("user", S, n_seq), params, "user_encoder", h, x, dout)
    t_ref = time.time() - t0
    row, n_bad, worst = first_bad_row(dx, r_dx.reshape(n_seq * S, d), mode)
    print("\nmany rows S=%d n_seq=%d (%d rows) %s: max|dout| %.3e, dx max|diff| %.3e, rows of dx outside the bound %d (first %s); "
          "device peak %.2f GB, GPU %.1f s, reference %.1f s" % (S, n_seq, n_seq * S, mode, float(np.abs(out - r_out).max()), worst,
                                                                n_bad, row, peak / 1e9, t_gpu, t_ref))
    assert peak < 4e9
    np.testing.assert_allclose(out, r_out, rtol=0, atol=TOL[mode]["score"])
    assert row is None, "dx: %d rows outside the bound, the first is row %d (sequence %d); the float reciprocal's first wrong row " \
                        "at S=%d was %d" % (n_bad, row, row // S, S, FIRST_WRONG[S])
    check_param_grads(layout, gflat, r_grads, mode, "S=%d" % S)


@gpu
def test_many_rows_fused_user_encoder():
    """The one-kernel user encoder (csrc/user64.hip, bf16x3, 33..64 slots) at the same 8.8 M rows: it does not go through
    E_DCTX; this pins its own indexing at that size."""
    S, n_seq, d, h, q, mode = 63, 140000, 8, 2, 4, "bf16x3"
    from pytorch_news_recommender_amd import _lib
    eng, flat, layout, params = make_engine(4, d, h, q, mode)
    assert eng._desc("user_encoder", n_seq, S, training=True).flags & _lib.NRMS_FLAG_FUSED_SEQ64
    rng = np.random.default_rng(1000 + S)
    x = rng.normal(0.2, 0.5, size=(n_seq, S, d)).astype(np.float32)
    dout = rng.normal(0.3, 1.0, size=(n_seq, d)).astype(np.float32)
    xd, dd = torch.from_numpy(x).cuda(), torch.from_numpy(dout).cuda()
    out = eng.encode_users(flat, xd, save=True)
    gflat = torch.zeros_like(flat)
    dx = eng.encode_users_backward(flat, gflat, xd, dd).cpu().numpy().reshape(n_seq * S, d)
    r_out, r_dx, r_grads = cached_reference(("user", S, n_seq), params, "user_encoder", h, x, dout)
    row, n_bad, worst = first_bad_row(dx, r_dx.reshape(n_seq * S, d), mode)
    print("\nmany rows fused S=%d: dx max|diff| %.3e, rows outside the bound %d (first %s)" % (S, worst, n_bad, row))
    np.testing.assert_allclose(out.cpu().numpy(), r_out, rtol=0, atol=TOL[mode]["score"])
    assert row is None, (n_bad, row)
    check_param_grads(layout, gflat, r_grads, mode, "fused S=%d" % S)


def ragged_ids(rng, n, L, V):
    """Right-padded titles of 1..L words, sequence 1 all padding, sequence 2 one word, every 97th all padding."""
    ids = rng.integers(1, V, size=(n, L), dtype=np.int64)
    lens = rng.integers(1, L + 1, size=n)
    lens[1::97] = 0
    if n > 2:
        lens[2] = 1
    ids[np.arange(L)[None, :] >= lens[:, None]] = 0
    return ids


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_many_rows_news_encoder(mode):
    """The same 9.0 M rows through the news encoder (vocab 4 096, NRMS_FLAG_PAD_ROW_ZERO, ragged titles): the token compaction,
    the grouped scatter of the table gradient and the capped grids of the pooling backward at 10 x the rows of any other test;
    the WHOLE table gradient is compared (a table row sums ~1 300 tokens, so a misplaced token row shows)."""
    S, n_seq, V, d, h, q = 30, 300000, 4096, 8, 2, 4
    eng, flat, layout, params = make_engine(V, d, h, q, mode, table_mean=0.25)
    eng.pad_row_zero = True
    rng = np.random.default_rng(77)
    ids = ragged_ids(rng, n_seq, S, V)
    dout = rng.normal(0.3, 1.0, size=(n_seq, d)).astype(np.float32)
    idd, dd = torch.from_numpy(ids).cuda(), torch.from_numpy(dout).cuda()
    out = eng.encode_titles(flat, idd, save=True)
    gflat = torch.zeros_like(flat)
    encode_titles_backward(eng, flat, gflat, idd, dd)
    eng.check_ids()
    r_out, _, r_grads = cached_reference(("news", S, n_seq), params, "news_encoder", h, ids, dout)
    table = "news_encoder.word_embedding.0.weight"
    got = layout.view(gflat, table).cpu().numpy()
    row, n_bad, worst = first_bad_row(got, r_grads[table], mode)
    print("\nmany rows news S=%d n_seq=%d %s: max|dout| %.3e, table gradient max|diff| %.3e (scale %.3e), rows outside the bound %d "
          "(first %s)" % (S, n_seq, mode, float(np.abs(out.cpu().numpy() - r_out).max()), worst, float(np.abs(r_grads[table]).max()),
                          n_bad, row))
    np.testing.assert_allclose(out.cpu().numpy(), r_out, rtol=0, atol=TOL[mode]["score"])
    assert not got[0].any()
    check_param_grads(layout, gflat, r_grads, mode, "news")


@gpu
def test_many_rows_fp16_news_encoder():
    """The default precision is not exempt: 300 000 titles of 30 words through the fused fp16 kernels (csrc/fused16.hip,
    fused16_bwd.hip), which do not use E_DCTX.  Bars: the fp16 ones of tests/test_hip_fuzz.py / tests/test_hip_fp16.py."""
    from pytorch_news_recommender_amd import _lib
    from tests.test_hip_fp16 import VEC_TOL
    S, n_seq, V, d, h, q = 30, 300000, 4096, 64, 2, 64
    eng, flat, layout, params = make_engine(V, d, h, q, "fp16", table_mean=0.1)
    eng.pad_row_zero = True
    assert eng._desc("news_encoder", n_seq, S, training=True).precision == _lib.NRMS_PRECISION_FP16
    rng = np.random.default_rng(78)
    ids = ragged_ids(rng, n_seq, S, V)
    dout = rng.normal(0.3, 1.0, size=(n_seq, d)).astype(np.float32)
    idd, dd = torch.from_numpy(ids).cuda(), torch.from_numpy(dout).cuda()
    torch.cuda.reset_peak_memory_stats()
    out = eng.encode_titles(flat, idd, save=True)
    gflat = torch.zeros_like(flat)
    encode_titles_backward(eng, flat, gflat, idd, dd)
    eng.check_ids()
    peak = torch.cuda.max_memory_allocated()
    r_out, _, r_grads = cached_reference(("news16", S, n_seq), params, "news_encoder", h, ids, dout, slice_seqs=2048)
    err = float(np.abs(out.cpu().numpy() - r_out).max())
    print("\nmany rows fp16 news: max|dout| %.3e (bar %.1e), device peak %.1f GB" % (err, VEC_TOL, peak / 1e9))
    assert err <= VEC_TOL
    floor = 1e-4 * max(float(np.abs(v).max()) for v in r_grads.values()) + 2e-6
    for name, ref in r_grads.items():
        got = layout.view(gflat, name).cpu().numpy()
        sc = float(np.abs(ref).max())
        if name.endswith("W_K.bias"):
            sc = max(sc, float(np.abs(r_grads[name.replace("W_K", "W_Q")]).max()))
        bad = float(np.abs(got - ref).max())
        print("  fp16 %-62s max|diff| %.3e scale %.3e" % (name, bad, sc))
        assert bad <= 8e-3 * sc + floor, (name, bad, sc)


# ---- 2. wide model, few rows ----------------------------------------------------------------------------------------------
def packed_offset(S, d, h):
    """Largest global offset (float2 units) PrefetchQKV keeps in 15 bits."""
    dk = d // h
    return (S - 1) * 3 * d // 2 + 3 * (dk // 2) - 1


WIDE = [
    (32, 672, 21, 64),       # the last width whose packed offset fits (31 295)
    (32, 704, 22, 64),       # the first that does not (32 783)
    (30, 768, 24, 200),      # the pretrained-vector width, 24 heads (33 455)
    (32, 1024, 32, 512),
    (17, 1024, 64, 256),     # packed, d_k = 16: 24 599 fits
    (33, 1024, 32, 256),     # 64 x 32 tiles: never packed
    (32, 1024, 16, 512),     # d_k = 64
    (64, 1024, 16, 512),     # 64 x 64 units
    (20, 1024, 8, 260),      # d_k = 128 and q_dim > 256: csrc/wide.hip (no NRMS_FLAG_PAD_ROW_ZERO: dense path)
]


def test_packed_offset_cases_sit_where_the_limit_is():
    assert packed_offset(32, 672, 21) == 31295 and packed_offset(32, 704, 22) == 32783 and packed_offset(30, 768, 24) == 33455
    assert packed_offset(17, 1024, 64) == 24599 and packed_offset(32, 1024, 32) > 0x7fff


def wide_case(S, d, h, q, mode, news, wo=False, mask_mode=0):
    n_seq, V = 6, 211
    eng, flat, layout, params = make_engine(V, d, h, q, mode, wo=wo, seed=5)
    rng = np.random.default_rng(S * 1000 + d)
    dout = rng.normal(0, 1, size=(n_seq, d)).astype(np.float32)
    lens = np.array([S, max(1, (2 * S) // 3), 1, 0, max(1, S - 2), S])         # one one-token and one empty sequence
    live = np.arange(S)[None, :] < lens[:, None]
    mask = live.astype(np.uint8) if mask_mode else None
    md = None if mask is None else torch.from_numpy(mask).cuda()
    dd = torch.from_numpy(dout).cuda()
    gflat = torch.zeros_like(flat)
    if news:
        eng.pad_row_zero = d // h <= 64                                          # wide.hip takes the dense path only
        ids = np.where(live, rng.integers(1, V, size=(n_seq, S)), 0).astype(np.int64)
        idd = torch.from_numpy(ids).cuda()
        out = eng.encode_titles(flat, idd, save=True, mask=md, mask_mode=mask_mode)
        encode_titles_backward(eng, flat, gflat, idd, dd, mask=md, mask_mode=mask_mode)
        eng.check_ids()
        r_out, r_dx, r_grads = reference(params, "news_encoder", h, ids, dout, mask=mask, mask_mode=mask_mode)
    else:
        x = rng.normal(0, 0.5, size=(n_seq, S, d)).astype(np.float32)
        xd = torch.from_numpy(x).cuda()
        out = eng.encode_users(flat, xd, save=True, mask=md, mask_mode=mask_mode)
        dx = eng.encode_users_backward(flat, gflat, xd, dd, mask=md, mask_mode=mask_mode)
        r_out, r_dx, r_grads = reference(params, "user_encoder", h, x, dout, mask=mask, mask_mode=mask_mode)
    err = float(np.abs(out.cpu().numpy() - r_out).max())
    what = "S=%d d=%d h=%d q=%d %s%s" % (S, d, h, q, "news" if news else "user", " W_O mask" if wo else "")
    print("\nwide %s %s: max|dout| %.3e (max|out| %.3f)" % (what, mode, err, float(np.abs(r_out).max())))
    np.testing.assert_allclose(out.cpu().numpy(), r_out, rtol=0, atol=TOL[mode]["score"])
    if not news:
        assert_grad_close(dx.cpu().numpy(), r_dx, mode, what + " dx")
    else:
        assert not layout.view(gflat, "news_encoder.word_embedding.0.weight")[0].any()
    worst = check_param_grads(layout, gflat, r_grads, mode, what)
    print("  worst gradient (relative to its tensor's scale): %s %.3e" % (max(worst, key=worst.get), max(worst.values())))


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("news", [True, False], ids=["news", "user"])
@pytest.mark.parametrize("S,d,h,q", WIDE, ids=["S%d_d%d_h%d_q%d" % c for c in WIDE])
def test_wide_model(S, d, h, q, news, mode):
    wide_case(S, d, h, q, mode, news)


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("S,d,h,q", [(32, 704, 22, 64), (30, 768, 24, 200)], ids=["S32_d704_h22", "S30_d768_h24"])
def test_wide_model_output_projection_and_masks(S, d, h, q, mode):
    """nrms_bert's user-encoder topology (W_O, pairwise and pooling masks) at a history of at most 32."""
    wide_case(S, d, h, q, mode, news=False, wo=True, mask_mode=3)


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_nrms_bert_768_wide_history_30(mode):
    """nrms_bert itself at the width of a pretrained encoder: E = 768, 24 user heads, histories of 30 (packed offset 33 455)."""
    from tests import test_hip_nrms_bert as tb
    shape = synth.BertShape(n_news=300, bert_embed_size=768, user_heads_num=24, query_vector_dim_large=200, batch_size=6,
                            history_len=30, n_candidates=4)
    params = synth.make_params_bert(shape, seed=41)
    batch = synth.make_batch_bert(shape, seed=42)
    model = tb.make_model(shape, params, precision=mode).train()
    scores, loss, grads = tb.fwd_bwd(model, batch)
    r_scores, r_loss, r_grads = tb.restate_grads(params, batch, shape.user_heads_num)
    live = batch["candidate_mask"] != 0
    t = tb.TOL[mode]
    err = float(np.abs(scores[live] - r_scores[live]).max())
    print("\nnrms_bert E=768 h=24 H=30 %s: max|dscore| %.3e (max|score| %.3f)" % (mode, err, float(np.abs(r_scores[live]).max())))
    assert err <= t["score"] and abs(loss - r_loss) <= t["score"]
    for n in params:
        tb.close(grads[n], r_grads[n], t, n)
