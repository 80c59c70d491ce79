"""Attribute-bag configuration with the reference's field names and defaults
(/root/reference/MIND_2020/config.py:5-89).  Only fields the NRMS hot path, its data feed and
its train/eval loop read are kept; ``__nrms__()`` adds the model hyper-parameters exactly as
the reference's entry scripts expect to call it (run_v0.py:50)."""
import torch


class Config(object):
    def __init__(self, model_name='NRMS', dataset='../MIND'):
        self.model_name = model_name
        self.data_path = './data_processed/'
        self.train_path = dataset + '/train/'
        self.dev_path = dataset + '/dev/'
        self.test_path = dataset + '/test/'
        self.small_train_path = dataset + '/small_train/'
        self.small_dev_path = dataset + '/small_dev/'

        self.word_embedding_pretrained = 'all_word_embedding_v3.npz'
        self.bert_embedding_pretrained = 'news_embeds_512.npz'    # nrms_bert: pretrained vector per news id (config.py:18)
        self.mode = 'large'                      # 'large' / 'demo' / 'synthetic'

        self.save_path = './save_model/'
        self.log_path = './logs/' + self.model_name
        self.train_data = 'train_datas.pkl'
        self.dev_data = 'dev_datas.pkl'
        self.test_data = 'test_datas.pkl'

        self.n_words_title = 20                  # title length L (config.py:30)
        self.n_words_abst = 40
        self.history_len = 50                    # H
        self.sample_size = 5                     # negatives per positive: C = sample_size + 1 in training
        self.max_candidate_size = 300            # C in evaluation

        self.save_flag = True
        self.random_seed = 1998
        self.device = torch.device('cuda' if torch.cuda.is_available() else 'cpu')

        self.category_nums = 18 + 1              # nrms_naml: rows of the category table, row 0 = padding (config.py:45)
        self.n_words = 45800
        self.subcategory_nums = 293 + 1          # (config.py:47)
        self.cate_embed_size = 100               # (config.py:49)
        self.word_embed_size = 300
        self.num_epochs = 5
        self.eval_step = 5000
        self.batch_size = 512
        self.learning_rate = 1e-3
        self.dropout = 0.2
        self.require_improvement = 10000
        self.warm_up_steps = 500
        self.warm_up = False
        # train(): evaluate with train_eval.evaluate_metrics (AUC, MRR, nDCG@5, nDCG@10) instead of evaluate (AUC only);
        # checkpoints are still picked by the AUC
        self.eval_metrics = False
        # HIP path only: "fp32" (exact f32 MFMA), "bf16x3" (split-bf16 projections), "bf16", or "fp16" (fused
        # one-wavefront-per-title fp16 news encoder; the user encoder -- 3 % of the flops -- stays in bf16x3 unless
        # fp16_user_encoder is set, which keeps the scores inside the 1e-4 bar with margin)
        self.precision = "fp32"
        self.fp16_user_encoder = False
        # precision "fp16" only.  fp16_inference: run evaluation / get_news_vector (passes without a backward) on the fused fp16
        # kernels too; default False = those passes run in bf16x3, so eval scores are ~1e-6 and the AUC exact to the reference.
        # fp16_v1_news_encoder: nrms_v1's W_O news encoder on the fused fp16 kernels (2x faster; up to 1.6e-4 from fp32 on
        # 512-user batches -- outside the absolute 1e-4 bar, hence opt-in); default False = bf16x3
        self.fp16_inference = False
        self.fp16_v1_news_encoder = False
        # train_step's loss: "rowwise" = cross-entropy of each user over the user's own sample_size + 1 candidates (the reference's);
        # "pooled" = in-batch sampled softmax over the candidates of the whole batch (nrms_pooled_ce_fwd_bwd), with the logQ
        # correction where the feed provides ``candidate_logq`` (ClickFeed) unless logq_correction is False
        self.train_loss = "rowwise"
        self.logq_correction = True
        # HIP path only: when embedding row 0 (padding_idx) is all zeros, skip the padding tokens in the
        # Q|K|V projection and its weight gradient (identical results; include/nrms_hip.h NRMS_FLAG_PAD_ROW_ZERO)
        self.skip_padding_tokens = True
        # model "hierec" (model/hierec_hip.py; parity unpinned): weights of the sub-topic / topic terms of the hierarchical match
        self.hierec_lambda_sub = 0.7
        self.hierec_lambda_top = 0.15
        # model "graph" (model/graph_hip.py; parity unpinned): neighbours sampled per news slot when the batch carries no neighbor_rows
        self.graph_neighbors = 8
        # ... with an attached click graph (Model.attach_click_graph): rows reserved per batch for the vectors of sampled
        # neighbours that no slot of the batch shows (a fixed size: no per-batch host read).  A 512-user MIND-shaped batch
        # (28 160 slots x 8 draws over 130 k news) draws about twelve thousand distinct ones from a Zipf-skewed graph; beyond this many the
        # largest ids are dropped and counted (Model.check_click_graph)
        self.graph_extra_rows = 16384

    def __nrms__(self):
        self.news_feature_size = 800             # nrms_naml: 2 * word_embed_size + 2 * cate_embed_size (config.py:68)
        self.bert_embed_size = 512               # nrms_bert: width of the news-vector table (config.py:69)
        self.query_vector_dim_large = 400        # nrms_naml / nrms_bert user encoder (config.py:72)
        self.query_vector_dim = 200
        self.title_heads_num = 6
        self.num_attention_heads = 10
        self.user_heads_num = 8
