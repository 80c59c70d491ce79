"""Timing of one per-epoch resample of the training negatives (csrc/negsample.hip, nrms_negative_sample) over a synthetic log of
MIND-train size: about 2.2 M impressions, a Zipf-like shown length (mean about 37, capped at 300), S = 4 negatives per clicked item.
The exact counts of the generated log are in the record.

Three things are timed in the same run, alternating, best of three:
  * the kernel call (device events around nrms_negative_sample);
  * a torch restatement on the device: per block of impressions a padded [block, max_shown] matrix, `rand` keys, `argsort`, and
    the slices scattered into cand / clen (blocks sized to fit);
  * the numpy restatement on the host (tests/negsample_ref.py: one lexsort over the whole log), whose result the kernel's is
    compared with, byte for byte.  It takes about a minute per pass, so it runs `host_reps` times (default 1).
The bar: one resample must cost less than 1 % of the time an epoch over the same rows takes at the headline rate,
n_samples / users_per_s (users_per_s: the second argument; default the README's 166 000).

Usage: python tools/bench_negsample.py [out.json] [users_per_s] [n_imp] [host_reps]"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from pytorch_news_recommender_amd import _lib
from tests import negsample_ref as ref

S, CAP, ZIPF, P_POS, SEED = 4, 300, 1.125, 0.015, 20201107


def make_log(n_imp, rng):
    w = 1.0 / np.arange(1, CAP + 1) ** ZIPF
    lens = rng.choice(np.arange(1, CAP + 1), size=n_imp, p=w / w.sum()).astype(np.int64) + 1       # 2 .. 301 -> capped below
    lens = np.minimum(lens, CAP)
    imp_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(imp_ptr[-1])
    shown = rng.integers(1, 130000, size=nnz).astype(np.int32)
    label = (rng.random(nnz) < P_POS).astype(np.uint8)
    label[imp_ptr[:-1]] = 1                                                     # every impression has a click, as MIND-train's do
    return imp_ptr, shown, label


def torch_restatement(imp_ptr, shown, label, sample_ptr, cand, clen, block, gen_seed):
    """rand + argsort over padded blocks: the same slices of a uniform shuffle (other random numbers, so other negatives)."""
    dev = imp_ptr.device
    n_imp = imp_ptr.numel() - 1
    g = torch.Generator(device=dev).manual_seed(gen_seed)
    col = torch.arange(CAP, device=dev)
    for b0 in range(0, n_imp, block):
        b1 = min(n_imp, b0 + block)
        p0 = imp_ptr[b0:b1]
        n = imp_ptr[b0 + 1:b1 + 1] - p0
        valid = col[None, :] < n[:, None]
        at = torch.where(valid, p0[:, None] + col[None, :], torch.zeros_like(p0[:, None]))
        ids = shown[at].to(torch.int64)
        pos = valid & (label[at] != 0)
        neg = valid & ~pos
        key = torch.rand(b1 - b0, CAP, device=dev, generator=g)
        key = torch.where(neg, key, torch.full_like(key, 2.0))
        ranked = torch.gather(ids, 1, torch.argsort(key, dim=1))                # negatives in shuffle order, then the rest
        n_neg = neg.sum(1)
        # positives in shown order -> rows; p = ordinal of the positive inside its impression
        where = torch.nonzero(pos)                                              # row-major: impression, then position
        imp, p = where[:, 0], (torch.cumsum(pos, 1) - 1)[pos]
        rows = sample_ptr[b0] + torch.arange(where.shape[0], device=dev)
        cnt = torch.clamp(n_neg[imp] - p * S, 0, S)
        slot = torch.arange(S, device=dev)
        take = torch.clamp(p[:, None] * S + slot[None, :], max=CAP - 1)
        negs = torch.where(slot[None, :] < cnt[:, None], ranked[imp[:, None], take], torch.zeros_like(take))
        cand[rows, 0] = ids[pos]
        cand[rows, 1:] = negs
        clen[rows] = 1 + cnt


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    users_per_s = float(sys.argv[2]) if len(sys.argv) > 2 else 166000.0
    n_imp = int(sys.argv[3]) if len(sys.argv) > 3 else 2200000
    host_reps = int(sys.argv[4]) if len(sys.argv) > 4 else 1
    if not torch.cuda.is_available():
        raise SystemExit("bench_negsample: no GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda")
    lib = _lib.load()
    imp_ptr, shown, label = make_log(n_imp, np.random.default_rng(SEED))
    sample_ptr = ref.sample_ptr_of(imp_ptr, label)
    nnz, n_samples = int(imp_ptr[-1]), int(sample_ptr[-1])
    lens = np.diff(imp_ptr)
    d = {k: torch.from_numpy(v).to(dev) for k, v in dict(imp_ptr=imp_ptr, shown=shown, label=label, sample_ptr=sample_ptr).items()}
    cand = torch.empty(n_samples, S + 1, dtype=torch.int64, device=dev)
    clen = torch.empty(n_samples, dtype=torch.int64, device=dev)
    cand_t, clen_t = torch.empty_like(cand), torch.empty_like(clen)
    n_bad = torch.zeros(1, dtype=torch.int32, device=dev)
    need = int(lib.nrms_negative_sample_workspace_bytes(C.c_int64(n_imp), C.c_int64(nnz), S))
    ws = torch.empty(need // 4, dtype=torch.int32, device=dev)

    def kernel(seed):
        rc = lib.nrms_negative_sample(C.c_int64(n_imp), _lib.ptr(d["imp_ptr"]), _lib.ptr(d["shown"]), _lib.ptr(d["label"]), _lib.ptr(d["sample_ptr"]),
                                      S, ref.MAX_SHOWN, C.c_uint64(seed), _lib.ptr(cand), _lib.ptr(clen), _lib.ptr(n_bad), _lib.ptr(ws),
                                      C.c_size_t(need), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, "nrms_negative_sample")

    def event_ms(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    block = 65536
    restate = lambda r: torch_restatement(d["imp_ptr"], d["shown"], d["label"], d["sample_ptr"], cand_t, clen_t, block, r)
    kernel(0), restate(0)                                                       # warm-up: code objects, allocator
    torch.cuda.synchronize()
    t_kernel, t_torch, t_host = [], [], []
    want = same = None
    for r in range(3):
        t_kernel.append(event_ms(lambda: kernel(ref.epoch_seed(SEED, r))))
        t_torch.append(event_ms(lambda: restate(r)))
        if r < host_reps:
            t = time.perf_counter()
            want = ref.negative_sample(imp_ptr, shown, label, S, ref.epoch_seed(SEED, r))
            t_host.append((time.perf_counter() - t) * 1e3)
            same = bool(np.array_equal(cand.cpu().numpy(), want[0]) and np.array_equal(clen.cpu().numpy(), want[1]))
    torch_rows_ok = bool(torch.equal(cand_t[:, 0], cand[:, 0]) and torch.equal(clen_t, clen))
    epoch_s = n_samples / users_per_s
    best = min(t_kernel)
    out = dict(tool="bench_negsample", device=torch.cuda.get_device_name(0), S=S, max_shown=ref.MAX_SHOWN,
               log=dict(n_imp=n_imp, nnz=nnz, n_samples=n_samples, mean_shown=round(float(lens.mean()), 2), max_shown=int(lens.max()),
                        longer_than_64=int((lens > 64).sum()), zipf=ZIPF, p_pos=P_POS, hbm_mb=round((8 * 2 * (n_imp + 1) + 5 * nnz) / 1e6, 1)),
               kernel_ms=[round(v, 3) for v in t_kernel], torch_restatement_ms=[round(v, 3) for v in t_torch],
               host_numpy_ms=[round(v, 1) for v in t_host], torch_block=block,
               kernel_equals_host_restatement=same, torch_restatement_rows_and_lengths_equal=torch_rows_ok, n_bad=int(n_bad.item()),
               entries_per_s=round(nnz / best * 1e3), users_per_s=users_per_s, epoch_s=round(epoch_s, 3), bar_ms=round(epoch_s * 10, 3),
               resample_share_of_epoch=round(best / 1e3 / epoch_s, 6), bar_met=bool(best / 1e3 < 0.01 * epoch_s))
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
    if same is False:
        raise SystemExit("bench_negsample: the kernel's cand / clen differ from the host restatement")


if __name__ == "__main__":
    main()
