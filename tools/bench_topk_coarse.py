"""Timing of the fp16 shortlist with a certificate at B = 512 users, N = 130 000 news, d = 300, 50 excluded
ids, for (k, M) in {(10, 64), (10, 256), (100, 256)}, in one process:
  (i)   nrms_catalogue_pack_f16 over the catalogue, and the size of the packed copy;
  (ii)  nrms_topk_dot_coarse and its four stages (user, slices, merge, re-score + finish; the library's event timing);
  (iii) the served call, Model._recommend_coarse: the coarse call, the one nonzero, the exact call over the uncertified rows and
        the write-back, on Gaussian data and on a catalogue half of whose users see near-tied scores; beside nrms_topk_dot at the same k.
        With --parent_lib FILE (a libnrms_hip.so built from the parent commit) nrms_topk_dot is called in THAT library, in the same
        session; without it, in this tree's;
  (iv)  the certified share on Gaussian data at that size, and on the trained vectors of the synthetic corpus (nrms_v0 of the
        default size trained for --train_steps steps on SyntheticMind with 4 000 news; its dev users against its catalogue).
Device-event timing; every path is warmed up first, the paths alternate, each window is `reps` calls and every window's time is
kept: the record holds the minimum and the spread (max - min over the windows) of every path.  This is a record, not a gate.
Usage: python tools/bench_topk_coarse.py [B] [N] [reps] [--windows W] [--train_steps S] [--parent_lib FILE] [--json FILE]"""
import ctypes as C
import json
import os
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from pytorch_news_recommender_amd import _lib
from pytorch_news_recommender_amd.engine import ModelDims, NRMSEngine, _stream
from pytorch_news_recommender_amd.model import nrms_hip

CASES = ((10, 64), (10, 256), (100, 256))
STAGES = ("user", "slices", "merge", "rescore")


def event_ms(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def opt(argv, name, default, conv):
    if name in argv:
        i = argv.index(name)
        v = conv(argv[i + 1])
        del argv[i:i + 2]
        return v
    return default


def parent_top_k(path, dev):
    """nrms_topk_dot of another build of the library, with buffers of its own."""
    lib = C.CDLL(path, mode=os.RTLD_LOCAL | os.RTLD_DEEPBIND)       # its own kernels and launch stubs, whatever else is loaded
    for name in ("nrms_topk_dot_workspace_bytes", "nrms_topk_dot"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SIGNATURES[name]
    keep = {}

    def top_k(user, items, k, ex):
        B, d = user.shape
        N = items.shape[0]
        if k not in keep:
            need = lib.nrms_topk_dot_workspace_bytes(B, C.c_int64(N), d, k)
            keep[k] = (torch.empty((need + 7) // 8, dtype=torch.int64, device=dev), torch.empty(B, k, device=dev),
                       torch.empty(B, k, dtype=torch.int64, device=dev))
        ws, sc, ids = keep[k]
        rc = lib.nrms_topk_dot(B, C.c_int64(N), d, k, _lib.ptr(user), _lib.ptr(items), _lib.ptr(ex), ex.shape[1], _lib.ptr(sc),
                               _lib.ptr(ids), _lib.ptr(ws), C.c_size_t(ws.numel() * 8), _stream())
        assert rc == 0, rc
        return sc, ids

    return top_k


def trained_share(steps, dev):
    """The certified share of the dev users of a briefly trained nrms_v0 against its own catalogue (tools/train_parity.py's recipe)."""
    from pytorch_news_recommender_amd.config import Config
    from pytorch_news_recommender_amd.data_handler import DeviceFeed, SyntheticMind
    cfg = Config("nrms_hip")
    cfg.__nrms__()
    cfg.n_words_title, cfg.batch_size, cfg.dropout, cfg.learning_rate, cfg.max_candidate_size = 30, 256, 0.0, 1e-3, 40
    corpus = SyntheticMind(cfg, n_news=4000, seed=0)
    table = torch.from_numpy(np.asarray(corpus.embedding_table(cfg.word_embed_size), dtype=np.float32))
    torch.manual_seed(0)
    model = nrms_hip.Model(cfg, pretrained_word_embedding=table).to(dev).train()
    feed = DeviceFeed(cfg, corpus.train_samples(256 * 40), type=0, id2title_dict=corpus.id2title_dict, id2abst_dict=corpus.id2abst_dict,
                      batch_size=256, device=dev, shuffle=True, drop_last=True, seed=3)
    done, first, last = 0, None, None
    while done < steps:
        for b in feed:
            last = float(model.train_step(b)) / 256
            first = last if first is None else first
            done += 1
            if done >= steps:
                break
    model.eval()
    dev_samples, _ = corpus.eval_samples(1024, max_shown=30)
    users = DeviceFeed(cfg, dev_samples, type=1, id2title_dict=corpus.id2title_dict, id2abst_dict=corpus.id2abst_dict, batch_size=256,
                       device=dev)
    cat = model.encode_catalogue(users.titles)
    packed = model.pack_catalogue(cat)
    rec = {"steps": done, "loss_first": round(first, 4), "loss_last": round(last, 4), "n_news": int(cat.shape[0]), "n_users": 0,
           "stats": [float(v) for v in packed.stats.tolist()], "certified_share": {}, "equal_to_plain": True}
    for k, M in CASES:
        n_cert = n = 0
        for batch in users:
            ids, sc, cert = model.recommend(batch, k, cat, coarse=packed, coarse_shortlist=M, return_certified=True)
            p_ids, p_sc = model.recommend(batch, k, cat)
            rec["equal_to_plain"] &= bool(torch.equal(ids, p_ids) and torch.equal(sc.view(torch.int32), p_sc.view(torch.int32)))
            n_cert += int(cert.sum())
            n += int(cert.shape[0])
        rec["certified_share"]["k=%d M=%d" % (k, M)] = round(n_cert / max(1, n), 4)
        rec["n_users"] = n
    return rec


def main():
    argv = list(sys.argv[1:])
    out = opt(argv, "--json", None, str)
    parent_lib = opt(argv, "--parent_lib", None, str)
    windows = opt(argv, "--windows", 5, int)
    train_steps = opt(argv, "--train_steps", 240, int)
    B = int(argv[0]) if len(argv) > 0 else 512
    N = int(argv[1]) if len(argv) > 1 else 130000
    reps = int(argv[2]) if len(argv) > 2 else 20
    d, H = 300, 50
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    user = torch.randn(B, d, device=dev, generator=g)
    cat = torch.randn(N + 1, d, device=dev, generator=g)             # a model's catalogue: row 0 is the padding title's
    items = cat[1:]
    hist = torch.randint(0, N, (B, H), device=dev, generator=g)
    # "mixed": the second half of the width carries near-tied items, and every other user lives in that half (uncertifiable)
    cat_mix = cat.clone()
    cat_mix[1:, d // 2:] = torch.randn(1, d - d // 2, device=dev, generator=g) + 1e-3 * torch.randn(N, d - d // 2, device=dev, generator=g)
    user_mix = user.clone()
    user_mix[0::2, d // 2:] = 0
    user_mix[1::2, :d // 2] = 0
    eng = NRMSEngine(ModelDims(n_words=10, word_embed_size=d, num_attention_heads=10, query_vector_dim=200), dev)
    shim = types.SimpleNamespace(_engine=eng)                        # Model._recommend_coarse reads nothing else of the model
    base_topk = parent_top_k(parent_lib, dev) if parent_lib else (lambda u, i, k, ex: eng.top_k(u, i, k, ex))
    base = "parent" if parent_lib else "this tree"

    packed = eng.pack_catalogue(items)
    packed.source = (cat.data_ptr(), tuple(cat.shape))
    packed_mix = eng.pack_catalogue(cat_mix[1:])
    packed_mix.source = (cat_mix.data_ptr(), tuple(cat_mix.shape))
    serve = lambda u, c, p, k, M: nrms_hip.Model._recommend_coarse(shim, u, c, hist, k, M, p, True)

    paths = {"pack": lambda: eng.pack_catalogue(items)}
    for k in sorted({k for k, _ in CASES}):
        paths["nrms_topk_dot k=%d %s" % (k, base)] = lambda k=k: base_topk(user, items, k, hist)
    for k, M in CASES:
        paths["coarse call k=%d M=%d" % (k, M)] = lambda k=k, M=M: eng.top_k_coarse(user, packed, k, M, hist)
        paths["served k=%d M=%d gaussian" % (k, M)] = lambda k=k, M=M: serve(user, cat, packed, k, M)
        paths["served k=%d M=%d mixed" % (k, M)] = lambda k=k, M=M: serve(user_mix, cat_mix, packed_mix, k, M)
    for fn in paths.values():                                         # warm up every shape the timed windows use
        fn()
        fn()
    torch.cuda.synchronize()

    # what is timed is what it should be: the served list is nrms_topk_dot's, bit for bit
    equal, share = True, {}
    for k, M in CASES:
        for name, u, c, p in (("gaussian", user, cat, packed), ("mixed", user_mix, cat_mix, packed_mix)):
            ids, sc, cert = serve(u, c, p, k, M)
            w_sc, w_ids = base_topk(u, c[1:], k, hist)
            equal &= bool(torch.equal(ids, torch.where(w_ids >= 0, w_ids + 1, w_ids)) and torch.equal(sc.view(torch.int32), w_sc.view(torch.int32)))
            share["%s k=%d M=%d" % (name, k, M)] = round(float(cert.float().mean()), 4)
    print("served == nrms_topk_dot (%s): %s; certified share: %s" % (base, equal, share))

    ts = {name: [] for name in paths}
    for _ in range(windows):                                          # alternate the paths
        for name, fn in paths.items():
            ts[name].append(event_ms(fn, reps))
    # the stages, by the library's own events (a run of their own: the events add a little to every call)
    stages = {}
    for k, M in CASES:
        eng.timing(True)
        eng.timing_reset()
        for _ in range(reps):
            eng.top_k_coarse(user, packed, k, M, hist)
        torch.cuda.synchronize()
        row = {}
        for name in STAGES:
            ms, n = eng.timing_read("coarse_stage(%s)" % name)
            row[name] = round(ms / max(1, n), 4)
        ms, n = eng.timing_read("topk_dot_coarse")
        row["call"] = round(ms / max(1, n), 4)
        eng.timing(False)
        eng.timing_reset()
        stages["k=%d M=%d" % (k, M)] = row
        print("stages k=%d M=%d: %s" % (k, M, row))

    rec = {"date": time.strftime("%Y-%m-%d"), "device": torch.cuda.get_device_name(0), "B": B, "N": N, "d": d, "n_exclude": H,
           "reps": reps, "windows": windows, "baseline": base, "served_equals_nrms_topk_dot": equal, "packed_bytes": packed.nbytes,
           "stats": [float(v) for v in packed.stats.tolist()], "certified_share": share, "stages_ms": stages, "ms": {}, "spread_ms": {},
           "windows_ms": {}}
    for name, t in ts.items():
        rec["ms"][name] = round(min(t), 4)
        rec["spread_ms"][name] = round(max(t) - min(t), 4)
        rec["windows_ms"][name] = [round(v, 4) for v in t]
        print("%-40s %8.4f ms  spread %.4f  (windows %s)" % (name, min(t), max(t) - min(t), " ".join("%.4f" % v for v in t)))
    rec["ratio"] = {}
    for k, M in CASES:
        b0 = rec["ms"]["nrms_topk_dot k=%d %s" % (k, base)]
        for name in ("coarse call k=%d M=%d" % (k, M), "served k=%d M=%d gaussian" % (k, M), "served k=%d M=%d mixed" % (k, M)):
            rec["ratio"]["%s / nrms_topk_dot" % name] = round(rec["ms"][name] / b0, 4)
            print("%-40s / nrms_topk_dot k=%d (%s) = %.4f" % (name, k, base, rec["ratio"]["%s / nrms_topk_dot" % name]))
    if train_steps > 0:
        rec["trained"] = trained_share(train_steps, dev)
        print("trained vectors:", rec["trained"])
    if out:
        with open(out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
