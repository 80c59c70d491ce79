"""Timing of the pooled loss (csrc/poolce.hip, nrms_pooled_ce_fwd_bwd) at the training shape: B = 512 users, d = 300, R = 50 reject
entries per user, C = 5 and C = 2 candidates per user (2 560 and 1 024 pool columns), ids drawn from 65 000 news so that a few pool
columns repeat a positive or sit in a history, col_bias given, no mask.

Two things are timed per C in the same run, alternating, best of three windows of 20 calls (device events around each window):
  * the call (six kernels: scores, softmax, loss sum, duser, its slab sum, dcand);
  * a torch-eager fp32 restatement on the same device tensors: `mm`, the compare-mask over [B, M, R], `log_softmax`, two `mm`.
The call's loss and gradients are compared with the float64 restatement (tests/pooled_ce_ref.py) and with the torch restatement;
the largest differences are in the record.  The per-kernel times come from the library's timers in a window of their own.

Then the fp16 train step under the protocol of tools/bench_step.py (bench shape, dropout 0.2, three warm-up steps, ten timed steps
per window, device events), with the row-wise and with the pooled loss, alternating, best of three windows each: the share of the
step the pooled kernels take, by the library's timers and by the difference of the two step times.

The bar: the call is not slower than the torch restatement.  The share of the step is a record, whatever it is.

Usage: python tools/bench_pooled_ce.py [out.json]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from pytorch_news_recommender_amd import _lib, synth
from tests.pooled_ce_ref import pooled_ce

B, D, R, N_NEWS, SEED = 512, 300, 50, 65000, 20201108
KERNELS = ("pooled_ce_scores", "pooled_ce_softmax", "pooled_ce_loss_sum", "pooled_ce_duser", "pooled_ce_dcand")


def event_ms(fn, n):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / n


def bench_call(lib, Cn, rng, dev):
    M = B * Cn
    s = float(D) ** -0.25
    cand = (rng.standard_normal((M, D)) * s).astype(np.float32)
    user = (rng.standard_normal((B, D)) * s).astype(np.float32)
    ids = rng.integers(1, N_NEWS, size=M).astype(np.int64)
    rej = rng.integers(1, N_NEWS, size=(B, R)).astype(np.int64)
    rej[:, R - 8:] = 0                                                         # a padded history
    rej[np.arange(B), 0] = ids[(np.arange(B) * 7 % B) * Cn]                    # every user has clicked somebody else's positive
    ids[np.arange(1, B, 16) * Cn + Cn - 1] = ids[np.arange(1, B, 16) * Cn]     # some negatives repeat their row's positive
    bias = (rng.standard_normal(M) * 2.0).astype(np.float32)
    gs = 1.0 / B
    t = lambda a: torch.from_numpy(a).to(dev)
    cand_d, user_d, ids_d, rej_d, bias_d = t(cand), t(user), t(ids), t(rej), t(bias)
    need = int(lib.nrms_pooled_ce_workspace_bytes(B, Cn, D, R))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    loss = torch.zeros(1, dtype=torch.float32, device=dev)
    pairs = torch.zeros(1, dtype=torch.int64, device=dev)
    dcand, duser = torch.empty(M, D, dtype=torch.float32, device=dev), torch.empty(B, D, dtype=torch.float32, device=dev)

    def kernel():
        rc = lib.nrms_pooled_ce_fwd_bwd(B, Cn, D, R, _lib.ptr(cand_d), _lib.ptr(user_d), _lib.ptr(ids_d), None, _lib.ptr(rej_d), _lib.ptr(bias_d),
                                        C.c_float(gs), _lib.ptr(loss), _lib.ptr(dcand), _lib.ptr(duser), _lib.ptr(pairs), _lib.ptr(ws),
                                        C.c_size_t(need), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, "nrms_pooled_ce_fwd_bwd")

    own = torch.arange(B, device=dev) * Cn
    rows = torch.arange(B, device=dev)
    res = {}

    def restatement():
        z = user_d @ cand_d.T + bias_d[None, :]
        hit = ((ids_d[None, :, None] == rej_d[:, None, :]) & (rej_d[:, None, :] > 0)).any(-1)
        inc = (ids_d[None, :] != ids_d[own][:, None]) & ~hit
        inc[rows, own] = True
        lsm = torch.log_softmax(torch.where(inc, z, torch.full_like(z, float("-inf"))), dim=1)
        p = torch.exp(lsm)
        p[rows, own] -= 1.0
        g = torch.where(inc, p * gs, torch.zeros_like(p))
        res["loss"], res["duser"], res["dcand"], res["pairs"] = -lsm[rows, own].sum(), g @ cand_d, g.T @ user_d, inc.sum() - B

    kernel(), restatement()                                                    # warm-up: code objects, allocator, BLAS choices
    kernel(), restatement()
    torch.cuda.synchronize()
    t_kernel, t_torch = [], []
    for _ in range(3):
        t_kernel.append(event_ms(kernel, 20))
        t_torch.append(event_ms(restatement, 20))
    # the results: one call into zeroed cells against float64 and against the restatement
    loss.zero_(), pairs.zero_()
    kernel()
    restatement()
    torch.cuda.synchronize()
    ref = pooled_ce(cand, user, ids, Cn, None, rej, bias, float(np.float32(gs)))
    k_loss, k_du, k_dc = float(loss[0]), duser.cpu().numpy().astype(np.float64), dcand.cpu().numpy().astype(np.float64)
    same_pairs = int(pairs[0]) == ref["n_pairs"] == int(res["pairs"])
    # per-kernel times, a window of their own (the timers put two events around every launch)
    lib.nrms_timing_enable(1)
    lib.nrms_timing_reset()
    for _ in range(20):
        kernel()
    torch.cuda.synchronize()
    per_kernel = {}
    for name in KERNELS:
        ms, n = C.c_double(0.0), C.c_int64(0)
        lib.nrms_timing_read(name.encode(), C.byref(ms), C.byref(n))
        per_kernel[name] = round(ms.value / 20 * 1e3, 2)                       # microseconds per call (duser includes its slab sum)
    lib.nrms_timing_enable(0)
    lib.nrms_timing_reset()
    flop = 3 * 2.0 * B * M * D
    best_k, best_t = min(t_kernel), min(t_torch)
    return dict(C=Cn, M=M, workspace_mb=round(need / 1e6, 2), n_pairs=ref["n_pairs"], pairs_equal=bool(same_pairs),
                call_us=[round(v * 1e3, 2) for v in t_kernel], torch_us=[round(v * 1e3, 2) for v in t_torch],
                kernel_us=per_kernel, gflop=round(flop / 1e9, 3), call_tflops=round(flop / best_k / 1e9, 2),
                call_share_of_fp32_matrix_peak=round(flop / (best_k * 1e-3) / 157.3e12, 4),
                call_over_torch=round(best_k / best_t, 3), bar_met=bool(best_k <= best_t),
                loss=dict(float64=ref["loss_sum"], call=k_loss, torch=float(res["loss"])),
                max_abs_error_vs_float64=dict(call_duser=float(np.abs(k_du - ref["duser"]).max()), call_dcand=float(np.abs(k_dc - ref["dcand"]).max()),
                                              torch_duser=float(np.abs(res["duser"].cpu().numpy() - ref["duser"]).max()),
                                              torch_dcand=float(np.abs(res["dcand"].cpu().numpy() - ref["dcand"]).max()),
                                              max_abs_duser=float(np.abs(ref["duser"]).max()), max_abs_dcand=float(np.abs(ref["dcand"]).max())))


def bench_step(dev):
    from tests.test_hip_parity import make_model
    shape = synth.BENCH
    params = synth.make_params(shape, seed=0)
    batch = synth.make_batch(shape, seed=1)
    rng = np.random.default_rng(SEED)
    Bs, H, Cn = shape.batch_size, shape.history_len, shape.n_candidates
    batch["candidate_ids"] = rng.integers(1, N_NEWS, size=(Bs, Cn)).astype(np.int64)
    batch["browsed_ids"] = np.where(batch["browsed_mask"] != 0, rng.integers(1, N_NEWS, size=(Bs, H)), 0).astype(np.int64)
    batch["candidate_logq"] = np.log(rng.uniform(1e-6, 1e-3, size=(Bs, Cn))).astype(np.float32)
    tb = {k: torch.from_numpy(v).to(dev) for k, v in batch.items()}
    models = {}
    for loss in ("rowwise", "pooled"):
        m = make_model(shape, params, dropout=0.2, precision="fp16").train()
        m.config.train_loss = loss
        for _ in range(3):
            m.train_step(tb)
        models[loss] = m
    torch.cuda.synchronize()
    times = {k: [] for k in models}
    for _ in range(3):
        for k, m in models.items():
            times[k].append(event_ms(lambda: m.train_step(tb), 10))
    eng = models["pooled"].engine
    eng.timing(True)
    eng.timing_reset()
    for _ in range(5):
        last = models["pooled"].train_step(tb)
    torch.cuda.synchronize()
    timed = eng.timing_read("pooled_ce")[0] / 5
    eng.timing(False)
    eng.timing_reset()
    row = models["rowwise"].engine
    row.timing(True)
    row.timing_reset()
    for _ in range(5):
        models["rowwise"].train_step(tb)
    torch.cuda.synchronize()
    replaced = (row.timing_read("ce_loss")[0] + row.timing_read("click_bwd")[0]) / 5
    row.timing(False)
    row.timing_reset()
    best = {k: min(v) for k, v in times.items()}
    return dict(shape=dict(B=Bs, H=H, C=Cn, L=shape.n_words_title, d=shape.word_embed_size), precision="fp16", dropout=0.2,
                step_ms={k: [round(x, 4) for x in v] for k, v in times.items()}, users_per_s={k: round(Bs / v * 1e3) for k, v in best.items()},
                pooled_kernels_ms_per_step=round(timed, 4), rowwise_ce_loss_and_click_bwd_ms_per_step=round(replaced, 4),
                pooled_kernels_share_of_pooled_step=round(timed / best["pooled"], 4),
                step_time_pooled_over_rowwise=round(best["pooled"] / best["rowwise"], 4), pooled_loss_per_user=float(last) / Bs,
                overflow_steps=int(eng.grad_overflow_steps))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    if not torch.cuda.is_available():
        raise SystemExit("bench_pooled_ce: no GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda")
    lib = _lib.load()
    rng = np.random.default_rng(SEED)
    out = dict(tool="bench_pooled_ce", device=torch.cuda.get_device_name(0), B=B, d=D, R=R, calls=[bench_call(lib, Cn, rng, dev) for Cn in (5, 2)],
               step=bench_step(dev))
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
