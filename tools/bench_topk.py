"""Timing of catalogue-wide top-k retrieval (docs/EXPERIMENTS.md): the fused nrms_topk_dot (NRMSEngine.top_k) against the
torch composition it replaces -- torch.mm to a [B, N] fp32 matrix, scatter_ of -inf over the history ids, torch.topk --
at B = 512 users, N = 130 000 news (MIND's catalogue), d = 300, k in {10, 100}, 50 history ids per user; plus
Model.encode_catalogue of 130 000 titles.  Device-event timing; every shape is warmed up first and the two paths alternate.
Usage: python tools/bench_topk.py [B] [N] [reps]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from pytorch_news_recommender_amd.engine import ModelDims, NRMSEngine

PEAK_TF = 157.3        # fp32 MFMA peak of the MI355X (v_mfma_f32_32x32x2_f32)


def event_ms(fn, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    N = int(sys.argv[2]) if len(sys.argv) > 2 else 130000
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
    d, H = 300, 50
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    user = torch.randn(B, d, device=dev, generator=g)
    items = torch.randn(N, d, device=dev, generator=g)
    hist = torch.randint(0, N, (B, H), device=dev, generator=g)
    eng = NRMSEngine(ModelDims(n_words=10, word_embed_size=d, num_attention_heads=10, query_vector_dim=200), dev)

    def torch_path(k):
        s = torch.mm(user, items.T)
        s.scatter_(1, hist, float("-inf"))
        return torch.topk(s, k, dim=1)

    flops = 2.0 * B * N * d
    print("B=%d N=%d d=%d history=%d: user tiles of 32 -> catalogue re-read %d x %.0f MB = %.2f GB (Infinity Cache 256 MB)"
          % (B, N, d, H, (B + 31) // 32, N * d * 4 / 1e6, (B + 31) // 32 * N * d * 4 / 1e9))
    for k in (10, 100):
        fused = lambda: eng.top_k(user, items, k, hist)      # noqa: E731
        ref = lambda: torch_path(k)                          # noqa: E731
        for fn in (fused, ref):
            fn()
        torch.cuda.synchronize()
        tf, tt = [], []
        for _ in range(3):                                   # alternate the two paths
            tf.append(event_ms(fused, reps))
            tt.append(event_ms(ref, reps))
        for name, ts in (("fused nrms_topk_dot", tf), ("torch mm+scatter+topk", tt)):
            ms = min(ts)
            print("k=%-3d %-22s %8.3f ms (runs %s)  %10.0f users/s  %6.1f TF/s (%.0f %% of %.0f TF fp32 peak)"
                  % (k, name, ms, " ".join("%.3f" % t for t in ts), B / ms * 1e3, flops / ms / 1e9,
                     100 * flops / ms / 1e9 / PEAK_TF, PEAK_TF))

    # encode_catalogue of N titles (nrms_v0 at the MIND shape: 30 words, 300-wide, 10 heads)
    from pytorch_news_recommender_amd import synth
    from pytorch_news_recommender_amd.config import Config
    from pytorch_news_recommender_amd.model.nrms_hip import Model
    cfg = Config("nrms_hip")
    cfg.__nrms__()
    shape = synth.Shape(n_words=30000, word_embed_size=300, num_attention_heads=10, query_vector_dim=200, batch_size=8,
                        history_len=50, n_candidates=5, n_words_title=30)
    params = synth.make_params(shape, seed=1)
    model = Model(cfg, pretrained_word_embedding=params["news_encoder.word_embedding.0.weight"]).to(dev)
    titles = torch.randint(1, shape.n_words, (N, 30), device=dev, generator=g)
    titles[:, 20:] = 0
    model.encode_catalogue(titles)
    torch.cuda.synchronize()
    ms = min(event_ms(lambda: model.encode_catalogue(titles), 3) for _ in range(3))
    print("encode_catalogue %d titles x 30 words (precision %s): %.2f ms, %.0f titles/s" % (N, cfg.precision, ms, N / ms * 1e3))


if __name__ == "__main__":
    main()
