"""Timing of one per-epoch draw of catalogue negatives (csrc/catneg.hip, nrms_catalogue_negative_sample) over a synthetic click log of
MIND-train size: about 2.2 M rows (50 000 users with 10 .. 80 clicks of Zipf popularity over 130 000 news, the last click held out,
min_history 1), weights count ** 0.75 * 65536, S = 4 negatives per row.  The exact counts of the generated log are in the record.

Two things are timed in the same run, alternating, best of three:
  * the kernel call (device events around nrms_catalogue_negative_sample);
  * a torch draw WITHOUT rejection on the device: `torch.multinomial(weights, n_rows * S, replacement=True)` into cand -- what a
    caller would write first; it may repeat a news inside a row and hand a user a news they clicked.
The kernel's bytes are compared with the host restatement (tests/catneg_ref.py) on `check_rows` rows picked at random: a row is a
function of the row alone, so a sample of rows is a check of those rows.
The bar: one draw must cost less than 1 % of the time an epoch over the same rows takes at the headline train rate,
n_rows / users_per_s (users_per_s: the second argument; default the README's 166 000).

Usage: python tools/bench_catneg.py [out.json] [users_per_s] [n_users] [check_rows]"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from pytorch_news_recommender_amd import _lib
from tests import catneg_ref as ref

S, N_NEWS, ZIPF, POWER, SEED = 4, 130000, 1.05, 0.75, 20201107


def make_log(n_users, rng):
    """(row_key, row_user, row_pos, set_ptr, set_news, cum, n_clicks): the arrays data_handler.ClickFeed keeps, built directly."""
    lens = rng.integers(10, 81, size=n_users).astype(np.int64)
    user_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    p = 1.0 / np.arange(1, N_NEWS) ** ZIPF
    ids = rng.permutation(np.arange(1, N_NEWS))                                  # popularity is not the id order
    clicks = ids[rng.choice(N_NEWS - 1, size=int(user_ptr[-1]), p=p / p.sum())].astype(np.int64)
    user_of = np.repeat(np.arange(n_users, dtype=np.int64), lens)
    t = np.arange(len(clicks), dtype=np.int64) - user_ptr[user_of]
    train = t < (lens - 1)[user_of]                                              # the last click is held out
    rows = train & (t >= 1)
    pairs = np.unique(user_of[train] * N_NEWS + clicks[train])
    set_ptr = np.concatenate([[0], np.cumsum(np.bincount(pairs // N_NEWS, minlength=n_users))]).astype(np.int64)
    set_news = (pairs % N_NEWS).astype(np.int32)
    count = np.bincount(set_news, minlength=N_NEWS)
    w = np.floor(count.astype(np.float64) ** POWER * 65536).astype(np.int64)
    w[0] = 0
    return (np.flatnonzero(rows).astype(np.int64), user_of[rows].astype(np.int32), clicks[rows].astype(np.int32), set_ptr, set_news,
            ref.cum_of(w), len(clicks))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    users_per_s = float(sys.argv[2]) if len(sys.argv) > 2 else 166000.0
    n_users = int(sys.argv[3]) if len(sys.argv) > 3 else 50000
    check_rows = int(sys.argv[4]) if len(sys.argv) > 4 else 4000
    if not torch.cuda.is_available():
        raise SystemExit("bench_catneg: no GPU (a timing taken elsewhere says nothing)")
    dev = torch.device("cuda")
    lib = _lib.load()
    rng = np.random.default_rng(SEED)
    row_key, row_user, row_pos, set_ptr, set_news, cum, n_clicks = make_log(n_users, rng)
    n = len(row_key)
    d = [torch.from_numpy(a).to(dev) for a in (row_key, row_user, row_pos, set_ptr, set_news, cum)]
    weights = torch.from_numpy(np.diff(cum).astype(np.float32)).to(dev)
    cand = torch.empty(n, S + 1, dtype=torch.int64, device=dev)
    clen = torch.empty(n, dtype=torch.int64, device=dev)
    cand_t = torch.empty_like(cand)
    counters = torch.zeros(2, dtype=torch.int32, device=dev)
    need = int(lib.nrms_catalogue_negative_sample_workspace_bytes(C.c_int64(n), C.c_int64(N_NEWS), S))
    ws = torch.empty(need // 4, dtype=torch.int32, device=dev)

    def kernel(seed):
        counters.zero_()
        rc = lib.nrms_catalogue_negative_sample(C.c_int64(n), _lib.ptr(d[0]), _lib.ptr(d[1]), _lib.ptr(d[2]), C.c_int64(n_users), _lib.ptr(d[3]),
                                                _lib.ptr(d[4]), C.c_int64(N_NEWS), _lib.ptr(d[5]), S, C.c_uint64(seed), _lib.ptr(cand), _lib.ptr(clen),
                                                _lib.ptr(counters[0:]), _lib.ptr(counters[1:]), _lib.ptr(ws), C.c_size_t(need),
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
        _lib.check(rc, "nrms_catalogue_negative_sample")

    def multinomial(seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        cand_t[:, 0] = d[2]
        # (torch.multinomial takes at most 2^24 categories: 130 000 is inside)
        cand_t[:, 1:] = torch.multinomial(weights, n * S, replacement=True, generator=g).view(n, S)

    def event_ms(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    kernel(0), multinomial(0)                                                   # warm-up: code objects, allocator
    torch.cuda.synchronize()
    t_kernel, t_torch = [], []
    for r in range(3):
        t_kernel.append(event_ms(lambda: kernel(ref.epoch_seed(SEED, r))))
        t_torch.append(event_ms(lambda: multinomial(r)))
    n_short, n_bad = counters.tolist()
    pick = np.sort(rng.choice(n, size=min(check_rows, n), replace=False))
    want = ref.catalogue_negative_sample(row_key[pick], row_user[pick], row_pos[pick], set_ptr, set_news, cum, S, ref.epoch_seed(SEED, 2))
    at = torch.from_numpy(pick).to(dev)
    same = bool(np.array_equal(cand[at].cpu().numpy(), want[0]) and np.array_equal(clen[at].cpu().numpy(), want[1]))
    neg_t = cand_t[:, 1:]
    repeats_t = int((neg_t.sort(dim=1).values.diff(dim=1) == 0).any(dim=1).sum())
    epoch_s = n / users_per_s
    best = min(t_kernel)
    out = dict(tool="bench_catneg", device=torch.cuda.get_device_name(0), S=S, power=POWER,
               log=dict(n_users=n_users, n_clicks=n_clicks, n_rows=n, n_news=N_NEWS, set_entries=int(set_ptr[-1]), weighted_news=int((np.diff(cum) > 0).sum()),
                        zipf=ZIPF, hbm_mb=round((16 * n + 8 * (n_users + 1) + 4 * int(set_ptr[-1]) + 8 * (N_NEWS + 1)) / 1e6, 1)),
               kernel_ms=[round(v, 3) for v in t_kernel], torch_multinomial_ms=[round(v, 3) for v in t_torch],
               kernel_equals_host_restatement=same, checked_rows=len(pick), n_short=n_short, n_bad=n_bad,
               multinomial_rows_with_a_repeat=repeats_t, rows_per_s=round(n / best * 1e3), users_per_s=users_per_s, epoch_s=round(epoch_s, 3),
               bar_ms=round(epoch_s * 10, 3), draw_share_of_epoch=round(best / 1e3 / epoch_s, 6), bar_met=bool(best / 1e3 < 0.01 * epoch_s))
    line = json.dumps(out)
    print(line)
    if out_path:
        with open(out_path, "w") as f:
            f.write(line + "\n")
    if not same:
        raise SystemExit("bench_catneg: the kernel's cand / clen differ from the host restatement")


if __name__ == "__main__":
    main()
