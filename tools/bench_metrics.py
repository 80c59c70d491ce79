"""Timing of nrms_impression_metrics (docs/EXPERIMENTS.md): the kernel on a dev-sized input (376 471 impressions x 300
slots), next to nrms_impression_auc on the same input, and the ranking stage of test() -- scores of a batch to the
submission rank lists -- on the host (_cal_test, the code before the kernel) and on the GPU.
Usage: python tools/bench_metrics.py [n_imp] [n_rank_imp]     (kernel times: run under rocprofv3 --kernel-trace --stats)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pytorch_news_recommender_amd import _lib
from pytorch_news_recommender_amd.engine import _stream, impression_metrics
from pytorch_news_recommender_amd.train_eval import _cal_test


def event_ms(fn, reps=5):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    n_imp = int(sys.argv[1]) if len(sys.argv) > 1 else 376471
    n_rank = int(sys.argv[2]) if len(sys.argv) > 2 else 50000
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    g = torch.Generator(device=dev).manual_seed(0)
    scores = torch.rand(n_imp, 300, device=dev, generator=g)
    labels = (torch.rand(n_imp, 300, device=dev, generator=g) < 0.05).to(torch.uint8)
    for name, lens in (("lens=300", torch.full((n_imp,), 300, dtype=torch.int32, device=dev)),
                       ("lens~U[2,300]", torch.randint(2, 301, (n_imp,), dtype=torch.int32, device=dev, generator=g))):
        auc = torch.empty(n_imp, dtype=torch.float64, device=dev)
        t_auc = event_ms(lambda: lib.nrms_impression_auc(n_imp, 300, _lib.ptr(scores), _lib.ptr(labels), _lib.ptr(lens),
                                                         _lib.ptr(auc), _stream()))
        t_met = event_ms(lambda: impression_metrics(lib, dev, scores, labels, lens))
        t_rk = event_ms(lambda: impression_metrics(lib, dev, scores, labels, lens, ranks=True))
        print("%-14s %d x 300: impression_auc %.3f ms, impression_metrics %.3f ms (with ranks %.3f ms)"
              % (name, n_imp, t_auc, t_met, t_rk))

    # ranking stage of test(): 512-impression batches of device scores -> rank lists on the host
    rng = np.random.default_rng(1)
    shown = rng.integers(2, 301, n_rank)
    batches = [torch.from_numpy(rng.standard_normal((min(512, n_rank - b), 300)).astype(np.float32)).to(dev)
               for b in range(0, n_rank, 512)]
    torch.cuda.synchronize()

    def host():
        out, k = [], 0
        for s in batches:
            sc = s.cpu().numpy()
            out.extend(_cal_test(sc[i], int(shown[k + i])) for i in range(len(sc)))
            k += len(sc)
        return out

    def gpu():
        out, k = [], 0
        for s in batches:
            nums = [int(n) for n in shown[k:k + len(s)]]
            lens = torch.tensor(nums, dtype=torch.int32).to(dev)
            lab = torch.zeros(s.shape, dtype=torch.uint8, device=dev)
            rk = impression_metrics(lib, dev, s, lab, lens, ranks=True)["ranks"].cpu().numpy()
            out.extend(rk[i, :n].tolist() for i, n in enumerate(nums))
            k += len(s)
        return out

    res = {}
    for name, fn in (("gpu", gpu), ("host", host), ("gpu", gpu)):
        t0 = time.perf_counter()
        r = fn()
        res[name] = (time.perf_counter() - t0, r)
    assert res["gpu"][1] == res["host"][1]
    print("test() ranking stage, %d impressions (shown ~ U[2,300]): host _cal_test %.2f s, GPU kernel %.3f s (identical lists)"
          % (n_rank, res["host"][0], res["gpu"][0]))


if __name__ == "__main__":
    main()
