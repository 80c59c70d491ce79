"""CLI entry with the reference's flags (/root/reference/MIND_2020/run_v0.py:15-28):

    python -m pytorch_news_recommender_amd.run_v0 --model nrms_hip --dataset synthetic
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m pytorch_news_recommender_amd.run_v0 ...

``--model nrms_bert`` (the reference's ``model/nrms.py``, NRMS over pretrained per-news vectors) also reads
config.data_path + config.bert_embedding_pretrained; ``--dataset synthetic`` writes topic-correlated vectors there.
``--dataset large|demo`` reads what the reference's preprocessing leaves under config.data_path
(idx_train_datas.pkl / idx_dev_datas.pkl, news_title.pkl or news_words.csv, dev_behaviors.csv:
data_handler.py:43-135, train_eval.py:36-39); ``--dataset synthetic`` fabricates a MIND-shaped corpus (no
data ships offline).  ``--batch_size`` (not a reference flag; its scripts hard-code 512 / 256, run_v0.py:44,
run_demo.py:28) lets BASELINE config 0 (batch 32) run through the same entry.
"""
import argparse
import inspect
import os
import time
from importlib import import_module

import numpy as np
import torch
from torch.utils.data import DataLoader

from . import parallel
from .config import Config
from .data_handler import ClickFeed, DeviceFeed, ImpressionFeed, MyDataset, SyntheticMind, load_dataset, read_dev_labels
from .model import Model
from .train_eval import (evaluate_retrieval, evaluate_retrieval_request, recommend, recommend_deep, recommend_request,
                         recommend_sections, test, train)

# rank r adds r * this to its dropout seeds (FlatHipModel._next_seed), so that the ranks of a data-parallel job draw unrelated masks
DROPOUT_RANK_SALT = 0x632BE59BD9B4E019


def build_parser():
    parser = argparse.ArgumentParser(description='MIND')
    parser.add_argument('--model', type=str, required=True, help='choose the proper model')
    parser.add_argument('--dataset', default='large', type=str, help='large | demo | synthetic')
    parser.add_argument('--test', default=False, type=bool, help='run the test dataset')
    parser.add_argument('--n_GPUs', type=int, default=1, help='number of GPUs (one process each: use torchrun)')
    parser.add_argument('--load', type=str, default=None, help='load the pretrained model ckpt file')
    parser.add_argument('--description', type=str, default=None, help='description of the experiment')
    parser.add_argument('--epochs', type=int, default=None)
    parser.add_argument('--max_batches', type=int, default=None)
    parser.add_argument('--synthetic_users', type=int, default=20480)
    parser.add_argument('--batch_size', type=int, default=512)
    parser.add_argument('--precision', type=str, default=None, help='fp32 | bf16x3 | bf16 | fp16 (HIP path)')
    parser.add_argument('--num_workers', type=int, default=6)
    parser.add_argument('--feed', type=str, default='device', help="device: batches assembled in HBM from a resident news "
                        "table (DeviceFeed); loader: the reference's DataLoader(MyDataset) with --num_workers processes")
    parser.add_argument('--data_path', type=str, default=None, help='overrides config.data_path (./data_processed/)')
    parser.add_argument('--metrics', action='store_true', help='evaluate on AUC, MRR, nDCG@5 and nDCG@10 (config.eval_metrics)')
    parser.add_argument('--save_path', type=str, default=None, help='overrides config.save_path (./save_model/)')
    parser.add_argument('--recommend', type=int, default=None, metavar='K', help='finally write the top K news of the whole '
                        'catalogue per impression: dev split with the trained weights, or with --test the test split with '
                        'the checkpoint --test loaded (nrms_v0 / nrms_v1 models)')
    parser.add_argument('--retrieval_metrics', type=str, default=None, metavar='K[,K...]', help='finally print Recall@K, nDCG@K, MRR '
                        'and the median rank of the held-out clicks in the ranking of the whole catalogue (any K >= 1: ranks are '
                        'exact at any depth): dev split with the trained weights, or with --test the test split (models whose '
                        'catalogue score is a plain dot product)')
    parser.add_argument('--graph', type=str, default='induced', choices=('induced', 'global'), help="--model graph: where a news "
                        "slot's neighbours come from.  induced: the click graph of the batch itself (host sampler); global: the "
                        "click graph of the whole training feed, resident in HBM, sampled by the HIP sampler (needs --feed device)")
    parser.add_argument('--negatives', type=str, default='fixed', choices=('fixed', 'epoch', 'catalogue', 'adaptive'), help="where a training row's "
                        "negatives come from.  fixed: drawn once, with the data set (the reference's offline preprocessing); epoch: redrawn "
                        "at the start of every epoch from the impression's own non-clicked news, on the device (ImpressionFeed); "
                        "catalogue: training on a click log without impressions, the negatives redrawn every epoch from the whole "
                        "catalogue by smoothed popularity, on the device (ClickFeed); adaptive: the same click log, the negatives redrawn "
                        "every epoch from the model's own softmax over the catalogue (hard negatives; models whose catalogue score is a "
                        "plain dot product).  epoch, catalogue and adaptive need --dataset synthetic and --feed device")
    parser.add_argument('--negative_temperature', type=float, default=1.0, metavar='T', help='--negatives adaptive: a news is drawn with '
                        'probability softmax(score / T); T > 0, large T approaches the uniform draw, small T the hardest negatives')
    parser.add_argument('--negative_power', type=float, default=0.75, metavar='P', help='--negatives catalogue: a news is drawn with '
                        'weight (number of users who clicked it) ** P; 0 = uniform over the catalogue')
    parser.add_argument('--loss', type=str, default='rowwise', choices=('rowwise', 'pooled'), help="the training loss.  rowwise: each user "
                        "against the user's own sample_size + 1 candidates (the reference's cross-entropy); pooled: each user against the "
                        "candidates of the whole batch (in-batch sampled softmax; with --negatives catalogue the scores are corrected by "
                        "the log of each news's probability of being in the pool)")
    parser.add_argument('--no_logq', action='store_true', help='--loss pooled: leave the log-probability correction out')
    parser.add_argument('--diversity', type=float, default=None, metavar='LAMBDA', help='--recommend: re-rank the list for diversity by '
                        'maximal marginal relevance over a shortlist, LAMBDA * relevance - (1 - LAMBDA) * largest cosine to the news '
                        'picked so far (0 <= LAMBDA <= 1; 1 = the plain list), and print ILD@K and catalogue coverage of the plain '
                        'and of the re-ranked list')
    parser.add_argument('--shortlist', type=int, default=None, metavar='M', help='--diversity: the number of best news the re-ranking '
                        'picks from (K <= M <= 256; default min(256, 4 K))')
    parser.add_argument('--retrieval_nll', type=str, default=None, metavar='T[,T...]', help='with --retrieval_metrics: also print the '
                        'held-out negative log-likelihood of the clicked news under softmax(score / T) over the whole catalogue, one '
                        'nll@T figure per temperature (up to 8, each > 0; with --popularity_prior the prior is part of the logit; not '
                        'with --catalogue_window)')
    parser.add_argument('--popularity_prior', type=float, default=None, metavar='ALPHA', help='--negatives catalogue / adaptive: add the '
                        "per-news prior ALPHA * log(1 + the number of training users who clicked the news) to every catalogue score of "
                        '--recommend (with or without --diversity) and --retrieval_metrics (0 = none; held-out clicks are not counted)')
    parser.add_argument('--catalogue_window', type=int, default=None, metavar='SPAN', help='--negatives catalogue / adaptive: give the '
                        'synthetic click log ticks, and let --recommend and --retrieval_metrics see, per held-out click, only the news '
                        'first clicked in the SPAN ticks up to the moment of that click (SPAN >= 1): the news that were live then')
    parser.add_argument('--coarse_catalogue', action='store_true', help='--recommend: serve through the fp16 shortlist with a '
                        'certificate (model.recommend(coarse=...)): the same file, bit for bit; prints the share of users whose list the '
                        'certificate covered (not with --diversity, --popularity_prior, --catalogue_window or --sections)')
    parser.add_argument('--coarse_shortlist', type=int, default=None, metavar='M', help='--coarse_catalogue: the news the fp16 pass '
                        'keeps per user (K <= M <= 256; default min(256, max(64, 4 K)))')
    parser.add_argument('--recommend_deep', type=int, default=None, metavar='K', help='finally write the first K news of the ranking '
                        'of the whole catalogue per impression, 1 <= K <= 4096 (candidates for a re-ranker; pages of 256 chained on the '
                        'device): the file and the split of --recommend, which it replaces; works with --popularity_prior and '
                        '--catalogue_window, not with --diversity, --shortlist, --coarse_catalogue or --sections')
    parser.add_argument('--recommend_out', type=str, default=None, help='file name of --recommend / --recommend_deep (default '
                        'recommend_<model>_<time>.txt)')
    parser.add_argument('--sections', type=str, default=None, choices=('category', 'subcategory'), help='--recommend: write the front '
                        'page by section instead, the top K news of every category (or sub-category) per impression, as '
                        '"<impression> <section> [ids]" lines (models whose catalogue score is a plain dot product; not with --diversity)')
    parser.add_argument('--explain', type=int, default=None, metavar='M', help='--recommend: also write, per recommended news, the M '
                        "clicks of the user's history that contribute most to its score (1 <= M <= 8; model.explain), to "
                        '<recommend_out>.reasons; reads the final ids only, so it goes with --diversity, --popularity_prior, '
                        '--catalogue_window and --coarse_catalogue (not with --sections or --recommend_deep)')
    parser.add_argument('--only_categories', type=str, default=None, metavar='own|ID[,ID...]', help='--recommend / --retrieval_metrics: '
                        "serve and rank inside a per-user set of news categories (model.recommend_tagged / rank_targets_tagged).  own: "
                        "the categories of the user's own training clicks (a click log) or history; ID[,ID...]: the same category ids "
                        'for everybody.  Combines with --mute_categories (allow = only minus mute) and --popularity_prior; not with '
                        '--catalogue_window, --coarse_catalogue, --recommend_deep, --sections, --diversity, --retrieval_nll or --explain')
    parser.add_argument('--mute_categories', type=str, default=None, metavar='ID[,ID...]', help='--recommend / --retrieval_metrics: never '
                        'serve these news categories, and rank the held-out clicks among the others (see --only_categories)')
    parser.add_argument('--max_per_category', type=int, default=None, metavar='M', help='--recommend: at most M news of one category '
                        'in every list (model.recommend_capped: the exact ranking walked greedily, a news is taken while its '
                        'category has room; M >= 1).  Combines with --only_categories / --mute_categories (a closed category gets cap '
                        '0) and --popularity_prior; not with --diversity, --coarse_catalogue, --catalogue_window, --sections, '
                        '--recommend_deep or --explain')
    parser.add_argument('--seen_discount', type=float, default=None, metavar='BETA', help='--recommend / --retrieval_metrics: impression '
                        'discounting (model.recommend_adjusted / rank_targets_adjusted): a news the user was shown c times without a '
                        "click goes down by BETA * c for that user alone.  Needs a feed with a seen log (--dataset synthetic with "
                        '--negatives catalogue or adaptive).  Combines with --popularity_prior; not with --diversity, '
                        '--coarse_catalogue, --catalogue_window, --only_categories / --mute_categories, --max_per_category, '
                        '--retrieval_nll, --explain, --sections or --recommend_deep')
    parser.add_argument('--seen_slots', type=int, default=None, metavar='E', help='--seen_discount: at most E seen news per user are '
                        'discounted, the most-seen first (1 <= E <= 256; default 32)')
    parser.add_argument('--combine_filters', action='store_true', help='--recommend / --retrieval_metrics: serve and rank one request '
                        'through several catalogue filters at once (model.recommend_request / rank_targets_request): with this flag '
                        '--catalogue_window, --only_categories / --mute_categories, --seen_discount and --popularity_prior may be given '
                        'together.  Every other refusal of those flags stays (no --diversity, --coarse_catalogue, --max_per_category, '
                        '--retrieval_nll, --explain, --sections or --recommend_deep); without the flag they refuse each other as before')
    parser.add_argument('--request_max_per_category', type=int, default=None, metavar='M', help='--combine_filters --recommend K: at '
                        'most M news of one category in every list, through the request (model.recommend_request_capped: the capped '
                        'walk over the news that --catalogue_window, --only_categories / --mute_categories and --seen_discount leave '
                        'open; M >= 1).  --max_per_category stays the capped call of the plain list and refuses --combine_filters')
    return parser


def check_request_caps_args(args):
    """--request_max_per_category fails before any data is read or any step is trained: M >= 1, and the list of --combine_filters
    --recommend K to ration (--combine_filters checks the model and the paths a request does not compose with)."""
    if args.request_max_per_category is None:
        return
    if args.request_max_per_category < 1:
        raise SystemExit('--request_max_per_category M: M must be >= 1 (got %d)' % args.request_max_per_category)
    if not args.combine_filters or args.recommend is None:
        raise SystemExit('--request_max_per_category: caps the list of --combine_filters --recommend K (give both)')


def check_seen_args(args):
    """--seen_discount / --seen_slots fail before any data is read or any step is trained: a finite BETA, 1 <= E <= 256, a list or a
    metric to apply them to, a feed with a seen log, a model that serves with per-user adjustments, and none of the paths the
    adjusted kernels do not have.  Returns (beta, slots) or None."""
    if args.seen_discount is None:
        if args.seen_slots is not None:
            raise SystemExit('--seen_slots E: the slots of --seen_discount BETA (give --seen_discount)')
        return None
    slots = 32 if args.seen_slots is None else args.seen_slots
    if not np.isfinite(args.seen_discount):
        raise SystemExit('--seen_discount BETA: BETA must be finite (got %r)' % args.seen_discount)
    if not 1 <= slots <= 256:
        raise SystemExit('--seen_slots E: E must be in [1, 256] (got %d)' % slots)
    if args.recommend is None and args.retrieval_metrics is None:
        raise SystemExit('--seen_discount: discounts the list of --recommend K and the ranks of --retrieval_metrics K (give one of them)')
    together = getattr(args, 'combine_filters', False)          # --combine_filters: the window and the categories go with the discount
    for other, on in (('--diversity', args.diversity is not None or args.shortlist is not None),
                      ('--coarse_catalogue', args.coarse_catalogue or args.coarse_shortlist is not None),
                      ('--catalogue_window', args.catalogue_window is not None and not together),
                      ('--only_categories', args.only_categories is not None and not together),
                      ('--mute_categories', args.mute_categories is not None and not together),
                      ('--max_per_category', args.max_per_category is not None), ('--retrieval_nll', args.retrieval_nll is not None),
                      ('--explain', args.explain is not None), ('--sections', args.sections is not None),
                      ('--recommend_deep', args.recommend_deep is not None)):
        if on:
            raise SystemExit('--seen_discount: the adjusted calls serve and rank the plain or the biased list only (drop %s)' % other)
    if args.dataset != 'synthetic' or args.negatives not in ('catalogue', 'adaptive'):
        raise SystemExit('--seen_discount: needs a feed with a seen log: --dataset synthetic with --negatives catalogue or adaptive')
    if args.test:
        raise SystemExit('--seen_discount: goes with the --recommend / --retrieval_metrics of a training run (drop --test)')
    from .model import ALIASES
    name = args.model.lower()
    module = import_module('.model.' + ALIASES.get(name, name), __package__)
    if not getattr(module.Model, 'CATALOGUE_ADJUST', False):
        raise SystemExit('--seen_discount: model %r cannot serve with per-user score adjustments (its catalogue score is no plain dot '
                         'product over a row-ordered catalogue)' % args.model)
    return float(args.seen_discount), slots


def check_combine_args(args):
    """--combine_filters fails before any data is read or any step is trained: a list or a metric to serve through the request calls,
    and none of the paths a request does not compose with."""
    if not args.combine_filters:
        return
    if args.recommend is None and args.retrieval_metrics is None:
        raise SystemExit('--combine_filters: combines the filters of --recommend K and --retrieval_metrics K (give one of them)')
    for other, on in (('--diversity', args.diversity is not None or args.shortlist is not None),
                      ('--coarse_catalogue', args.coarse_catalogue or args.coarse_shortlist is not None),
                      ('--max_per_category', args.max_per_category is not None), ('--retrieval_nll', args.retrieval_nll is not None),
                      ('--explain', args.explain is not None), ('--sections', args.sections is not None),
                      ('--recommend_deep', args.recommend_deep is not None)):
        if on:
            raise SystemExit('--combine_filters: a request composes a time window, categories, the seen-news discount and the prior '
                             'only (drop %s)' % other)
    from .model import ALIASES
    name = args.model.lower()
    module = import_module('.model.' + ALIASES.get(name, name), __package__)
    if not getattr(module.Model, 'CATALOGUE_ADJUST', False):
        raise SystemExit('--combine_filters: model %r cannot serve a request (its catalogue score is no plain dot product over a '
                         'row-ordered catalogue)' % args.model)


def check_caps_args(args):
    """--max_per_category fails before any data is read or any step is trained: M >= 1, the list of --recommend, a model that
    serves with per-category caps, and none of the paths the capped kernels do not have."""
    if args.max_per_category is None:
        return
    if args.max_per_category < 1:
        raise SystemExit('--max_per_category M: M must be >= 1 (got %d)' % args.max_per_category)
    if args.recommend is None:
        raise SystemExit('--max_per_category: caps the list of --recommend K (give --recommend)')
    for other, on in (('--diversity', args.diversity is not None or args.shortlist is not None),
                      ('--coarse_catalogue', args.coarse_catalogue or args.coarse_shortlist is not None),
                      ('--catalogue_window', args.catalogue_window is not None), ('--sections', args.sections is not None),
                      ('--recommend_deep', args.recommend_deep is not None), ('--explain', args.explain is not None)):
        if on:
            raise SystemExit('--max_per_category: the capped call serves the plain or the biased list only (drop %s)' % other)
    from .model import ALIASES
    name = args.model.lower()
    module = import_module('.model.' + ALIASES.get(name, name), __package__)
    if not getattr(module.Model, 'CATALOGUE_CAPS', False):
        raise SystemExit('--max_per_category: model %r cannot serve with per-category caps (its catalogue score is no plain dot '
                         'product over a row-ordered catalogue)' % args.model)


def check_tag_args(args):
    """--only_categories / --mute_categories fail before any data is read or any step is trained: category ids >= 0 (or "own"), a
    list or a metric to apply them to, a model that serves inside a tag set, and none of the paths the tagged kernels do not have.
    Returns (only, mute): only = None, 'own' or a tuple of ids; mute = None or a tuple of ids."""
    only = mute = None
    for flag, text in (('--only_categories', args.only_categories), ('--mute_categories', args.mute_categories)):
        if text is None:
            continue
        if flag == '--only_categories' and text == 'own':
            only = 'own'
            continue
        try:
            ids = tuple(int(v) for v in text.split(','))
        except ValueError:
            raise SystemExit('%s %s: category ids expected (got %r)' % (flag, 'own|ID[,ID...]' if flag == '--only_categories' else 'ID[,ID...]', text))
        if not ids or min(ids) < 0:
            raise SystemExit('%s: every category id must be >= 0 (got %r)' % (flag, text))
        if flag == '--only_categories':
            only = ids
        else:
            mute = ids
    if only is None and mute is None:
        return None, None
    flag = '--only_categories' if only is not None else '--mute_categories'
    if args.recommend is None and args.retrieval_metrics is None:
        raise SystemExit('%s: the categories of --recommend K and --retrieval_metrics K (give one of them)' % flag)
    for other, on in (('--catalogue_window', args.catalogue_window is not None and not getattr(args, 'combine_filters', False)),
                      ('--coarse_catalogue', args.coarse_catalogue or args.coarse_shortlist is not None),
                      ('--recommend_deep', args.recommend_deep is not None), ('--sections', args.sections is not None),
                      ('--diversity', args.diversity is not None or args.shortlist is not None),
                      ('--retrieval_nll', args.retrieval_nll is not None), ('--explain', args.explain is not None)):
        if on:
            raise SystemExit('%s: the tagged calls serve and rank the plain or the biased list only (drop %s)' % (flag, other))
    from .model import ALIASES
    name = args.model.lower()
    module = import_module('.model.' + ALIASES.get(name, name), __package__)
    if not getattr(module.Model, 'CATALOGUE_TAGS', False):
        raise SystemExit('%s: model %r cannot serve inside a per-user tag set (its catalogue score is no plain dot product over a '
                         'row-ordered catalogue)' % (flag, args.model))
    return only, mute


def check_explain_args(args):
    """--explain fails before any data is read or any step is trained: it explains the list of --recommend, M in [1, 8], and needs
    a model whose score is one additive-attention sum over the clicks."""
    if args.explain is None:
        return
    if args.recommend is None:
        raise SystemExit('--explain M: explains the list of --recommend K (give --recommend)')
    if not 1 <= args.explain <= 8:
        raise SystemExit('--explain M: M must be in [1, 8] (got %d)' % args.explain)
    if args.sections is not None:
        raise SystemExit('--explain: explains the one list of --recommend K, not a list per section (drop --sections)')
    from .model import ALIASES
    name = args.model.lower()
    module = import_module('.model.' + ALIASES.get(name, name), __package__)
    if not getattr(module.Model, 'CATALOGUE_EXPLAIN', False):
        raise SystemExit('--explain: model %r cannot split a score over the clicks of the history (its score is no single '
                         'additive-attention sum over them; nrms_v0 / nrms_v1 / nrms_naml / nrms_bert can)' % args.model)


def check_sections_args(args):
    """--sections fails before any data is read or any step is trained: it shapes the list of --recommend, has no re-ranking
    inside a section, and needs a model that selects per section."""
    if args.sections is None:
        return
    if args.recommend is None:
        raise SystemExit('--sections: the sections of the list of --recommend K (give --recommend)')
    if args.diversity is not None:
        raise SystemExit('--sections: no diversity re-ranking inside a section (drop --diversity)')
    from .model import ALIASES
    name = args.model.lower()
    module = import_module('.model.' + ALIASES.get(name, name), __package__)
    if not getattr(module.Model, 'CATALOGUE_SECTIONS', False):
        raise SystemExit('--sections: model %r cannot select per section (its catalogue score is no plain dot product)' % args.model)


def check_coarse_args(args):
    """--coarse_catalogue / --coarse_shortlist fail before any data is read or any step is trained: they serve the plain list of
    --recommend only."""
    if args.coarse_shortlist is not None and not args.coarse_catalogue:
        raise SystemExit('--coarse_shortlist M: the shortlist length of --coarse_catalogue (give --coarse_catalogue)')
    if not args.coarse_catalogue:
        return
    if args.recommend is None:
        raise SystemExit('--coarse_catalogue: serves the list of --recommend K (give --recommend)')
    for flag, on in (('--diversity', args.diversity is not None), ('--popularity_prior', args.popularity_prior is not None),
                     ('--catalogue_window', args.catalogue_window is not None), ('--sections', args.sections is not None)):
        if on:
            raise SystemExit('--coarse_catalogue: the certificate covers the plain top-k only (drop %s)' % flag)
    if args.coarse_shortlist is not None and not args.recommend <= args.coarse_shortlist <= 256:
        raise SystemExit('--coarse_shortlist M: M must be in [K, 256] (got M=%d, K=%d)' % (args.coarse_shortlist, args.recommend))


def check_deep_args(args):
    """--recommend_deep fails before any data is read or any step is trained: K in [1, 4096], the plain ranking only (no other
    list of --recommend beside it, no re-ranking, no fp16 shortlist, no sections), a model that can page through its ranking."""
    if args.recommend_deep is None:
        return
    if not 1 <= args.recommend_deep <= 4096:
        raise SystemExit('--recommend_deep K: K must be in [1, 4096] (got %d)' % args.recommend_deep)
    if args.recommend is not None:
        raise SystemExit('--recommend_deep: writes the list of --recommend at its own depth (drop --recommend)')
    for flag, on in (('--diversity', args.diversity is not None), ('--shortlist', args.shortlist is not None),
                     ('--coarse_catalogue', args.coarse_catalogue or args.coarse_shortlist is not None),
                     ('--sections', args.sections is not None)):
        if on:
            raise SystemExit('--recommend_deep: the plain ranking only, pages chained by a cursor (drop %s)' % flag)
    from .model import ALIASES
    name = args.model.lower()
    module = import_module('.model.' + ALIASES.get(name, name), __package__)
    if not (getattr(module.Model, 'CATALOGUE_RETRIEVAL', False) and getattr(module.Model, 'CATALOGUE_PAGING', False)):
        raise SystemExit('--recommend_deep: model %r cannot page through a ranking of the whole catalogue (nrms_v0 / nrms_v1 / '
                         'nrms_bert: a plain dot product over a row-ordered catalogue)' % args.model)


def check_recommend_args(args):
    """--recommend fails before any data is read or any step is trained: K in [1, 256], a model that can recommend; so do
    --diversity (needs --recommend, 0 <= LAMBDA <= 1, a model that re-ranks) and --shortlist (needs --diversity, K <= M <= 256)."""
    if args.diversity is not None:
        if args.recommend is None:
            raise SystemExit('--diversity LAMBDA: re-ranks the list of --recommend K (give --recommend)')
        if not 0.0 <= args.diversity <= 1.0:
            raise SystemExit('--diversity LAMBDA: LAMBDA must be in [0, 1] (got %r)' % args.diversity)
        from .model import ALIASES
        if ALIASES.get(args.model.lower(), args.model.lower()) in ('hierec_hip', 'graph_hip'):
            raise SystemExit('--diversity: model %r has no diversity re-ranking (its catalogue score is no plain dot product over a '
                             'row-ordered catalogue)' % args.model)
    if args.shortlist is not None:
        if args.diversity is None:
            raise SystemExit('--shortlist M: the candidate count of --diversity (give --diversity)')
        if not args.recommend <= args.shortlist <= 256:
            raise SystemExit('--shortlist M: M must be in [K, 256] (got M=%d, K=%d)' % (args.shortlist, args.recommend))
    if args.recommend is None:
        return
    if not 1 <= args.recommend <= 256:
        raise SystemExit('--recommend K: K must be in [1, 256] (got %d)' % args.recommend)
    from .model import ALIASES
    name = args.model.lower()
    module = import_module('.model.' + ALIASES.get(name, name), __package__)
    if not getattr(module.Model, 'CATALOGUE_RETRIEVAL', False):
        raise SystemExit('--recommend: model %r cannot recommend from the whole catalogue (nrms_v0 / nrms_v1 only)' % args.model)


def check_retrieval_args(args):
    """--retrieval_metrics fails before any data is read or any step is trained: integers >= 1, a model that can rank the
    catalogue.  Returns the cutoffs (None without the flag)."""
    if args.retrieval_metrics is None:
        return None
    try:
        ks = tuple(int(v) for v in args.retrieval_metrics.split(','))
    except ValueError:
        raise SystemExit('--retrieval_metrics K[,K...]: integers expected (got %r)' % args.retrieval_metrics)
    if not ks or min(ks) < 1:
        raise SystemExit('--retrieval_metrics K[,K...]: every K must be >= 1 (got %r)' % args.retrieval_metrics)
    if args.test and args.dataset != 'synthetic':
        raise SystemExit('--retrieval_metrics with --test: the MIND test split carries no click labels (synthetic data only)')
    from .model import ALIASES
    name = args.model.lower()
    module = import_module('.model.' + ALIASES.get(name, name), __package__)
    if not getattr(module.Model, 'CATALOGUE_RANKING', False):
        raise SystemExit('--retrieval_metrics: model %r cannot rank targets against the whole catalogue (its catalogue score is '
                         'no plain dot product)' % args.model)
    return ks


def check_nll_args(args):
    """--retrieval_nll fails before any data is read or any step is trained: up to 8 temperatures > 0, --retrieval_metrics to ride
    on, no time window (there is no windowed log-partition), a model whose catalogue score a softmax can be put on.  Returns the
    temperatures (None without the flag)."""
    if args.retrieval_nll is None:
        return None
    try:
        temps = tuple(float(v) for v in args.retrieval_nll.split(','))
    except ValueError:
        raise SystemExit('--retrieval_nll T[,T...]: numbers expected (got %r)' % args.retrieval_nll)
    if not 1 <= len(temps) <= 8 or not all(t > 0 for t in temps):
        raise SystemExit('--retrieval_nll T[,T...]: 1 to 8 temperatures, each > 0 (got %r)' % args.retrieval_nll)
    if args.retrieval_metrics is None:
        raise SystemExit('--retrieval_nll: the likelihood of the targets of --retrieval_metrics K (give it)')
    if args.catalogue_window is not None:
        raise SystemExit('--retrieval_nll: there is no log-partition inside a time window yet (drop --catalogue_window)')
    from .model import ALIASES
    name = args.model.lower()
    module = import_module('.model.' + ALIASES.get(name, name), __package__)
    if not getattr(module.Model, 'CATALOGUE_LIKELIHOOD', False):
        raise SystemExit('--retrieval_nll: model %r has no softmax over the whole catalogue (its catalogue score is not one dot '
                         'product per user)' % args.model)
    return temps


def check_prior_args(args):
    """--popularity_prior fails before any data is read or any step is trained: a finite ALPHA, a list or a metric to apply it to,
    a click log to count popularity in, and a model that takes a per-news prior."""
    if args.popularity_prior is None:
        return
    if not np.isfinite(args.popularity_prior):
        raise SystemExit('--popularity_prior ALPHA: ALPHA must be finite (got %r)' % args.popularity_prior)
    if args.recommend is None and args.recommend_deep is None and args.retrieval_metrics is None:
        raise SystemExit('--popularity_prior ALPHA: the prior of --recommend K, --recommend_deep K and --retrieval_metrics K (give one of them)')
    if args.negatives not in ('catalogue', 'adaptive'):
        raise SystemExit('--popularity_prior: popularity is counted in a click log (--negatives catalogue or adaptive, got %r)'
                         % args.negatives)
    from .model import ALIASES
    if ALIASES.get(args.model.lower(), args.model.lower()) in ('hierec_hip', 'graph_hip'):
        raise SystemExit('--popularity_prior: model %r takes no per-news prior (its catalogue score is no plain dot product over a '
                         'row-ordered catalogue)' % args.model)


def check_window_args(args):
    """--catalogue_window fails before any data is read or any step is trained: SPAN >= 1, a list or a metric to apply it to, a
    click log to take the ticks from, and a model that ranks a row-ordered catalogue."""
    if args.catalogue_window is None:
        return
    if args.catalogue_window < 1:
        raise SystemExit('--catalogue_window SPAN: SPAN must be >= 1 (got %d)' % args.catalogue_window)
    if args.recommend is None and args.recommend_deep is None and args.retrieval_metrics is None:
        raise SystemExit('--catalogue_window SPAN: the window of --recommend K, --recommend_deep K and --retrieval_metrics K (give one of them)')
    if args.negatives not in ('catalogue', 'adaptive'):
        raise SystemExit('--catalogue_window: the ticks belong to a click log (--negatives catalogue or adaptive, got %r)'
                         % args.negatives)
    if args.test:
        raise SystemExit('--catalogue_window with --test: the request times are those of the held-out clicks of a training run')
    if args.sections is not None:
        raise SystemExit('--catalogue_window: the front page by section has no time window (drop --sections)')
    from .model import ALIASES
    name = args.model.lower()
    module = import_module('.model.' + ALIASES.get(name, name), __package__)
    if not getattr(module.Model, 'CATALOGUE_RANKING', False):
        raise SystemExit('--catalogue_window: model %r takes no time window (its catalogue score is no plain dot product over a '
                         'row-ordered catalogue)' % args.model)


def check_graph_args(args):
    """--graph global fails before any data is read: the graph model on the device feed only."""
    if args.graph != 'global':
        return
    from .model import ALIASES
    if ALIASES.get(args.model.lower(), args.model.lower()) != 'graph_hip':
        raise SystemExit('--graph global: only --model graph samples from a click graph (got %r)' % args.model)
    if args.feed != 'device':
        raise SystemExit('--graph global: the click graph is built from the device feed (--feed device)')


def check_negatives_args(args):
    """--negatives epoch / catalogue / adaptive fail before any data is read: impressions with labels, or a click log, to train on
    exist for the synthetic corpus only (reading MIND's behaviors.tsv is out of scope), the log lives in the device feed, and --test
    trains nothing.  adaptive also needs a model that can sample from its catalogue scores, and no logQ correction."""
    if args.negatives in ('catalogue', 'adaptive'):
        flag = '--negatives ' + args.negatives
        if args.dataset != 'synthetic':
            raise SystemExit('%s: a click log exists for --dataset synthetic only (got %r: its pickles hold '
                             'negatives that were drawn offline)' % (flag, args.dataset))
        if args.feed != 'device':
            raise SystemExit('%s: the click log is sampled in the device feed (--feed device)' % flag)
        if args.test:
            raise SystemExit('%s: --test trains nothing' % flag)
        if not args.negative_power >= 0.0:
            raise SystemExit('--negative_power P: P must be >= 0 (got %r)' % args.negative_power)
        if args.graph == 'global':
            raise SystemExit('%s: --graph global builds its click graph from history rows, which a click log does '
                             'not keep' % flag)
        if args.negatives == 'adaptive':
            if not (args.negative_temperature > 0.0 and np.isfinite(args.negative_temperature)):
                raise SystemExit('--negative_temperature T: T must be finite and > 0 (got %r)' % args.negative_temperature)
            from .model import ALIASES
            name = args.model.lower()
            module = import_module('.model.' + ALIASES.get(name, name), __package__)
            if not getattr(module.Model, 'CATALOGUE_SAMPLING', False):
                raise SystemExit('--negatives adaptive: model %r cannot sample negatives from its catalogue scores (its catalogue '
                                 'score is no plain dot product)' % args.model)
            if args.loss == 'pooled' and not args.no_logq:
                raise SystemExit('--negatives adaptive with --loss pooled: an adaptive draw has no fixed log q to correct by '
                                 '(give --no_logq)')
        return
    if args.negatives != 'epoch':
        return
    if args.dataset != 'synthetic':
        raise SystemExit('--negatives epoch: training impressions exist for --dataset synthetic only (got %r: its pickles hold '
                         'negatives that were drawn offline)' % args.dataset)
    if args.feed != 'device':
        raise SystemExit('--negatives epoch: the impression log is sampled in the device feed (--feed device)')
    if args.test:
        raise SystemExit('--negatives epoch: --test trains nothing')


def check_loss_args(args):
    """--loss pooled fails before any data is read: a model whose engine has the pooled loss, and a run that trains."""
    if args.loss != 'pooled':
        return
    from .model import ALIASES
    if ALIASES.get(args.model.lower(), args.model.lower()) in ('hierec_hip', 'graph_hip'):
        raise SystemExit('--loss pooled: model %r has no pooled loss (nrms_v0, nrms_v1, nrms_bert and nrms_naml have)' % args.model)
    if args.test:
        raise SystemExit('--loss pooled: --test trains nothing')


def main(argv=None):
    args = build_parser().parse_args(argv)
    check_deep_args(args)
    check_recommend_args(args)
    check_sections_args(args)
    check_coarse_args(args)
    check_explain_args(args)
    retrieval_ks = check_retrieval_args(args)
    retrieval_nll = check_nll_args(args)
    check_prior_args(args)
    check_combine_args(args)
    check_request_caps_args(args)
    check_window_args(args)
    tag_only, tag_mute = check_tag_args(args)
    check_caps_args(args)
    seen_discount = check_seen_args(args)
    check_graph_args(args)
    check_negatives_args(args)
    check_loss_args(args)
    rank, local_rank, world = parallel.init_process_group()
    torch.manual_seed(422)
    torch.cuda.manual_seed_all(422)
    model_name = args.model + '_' + (args.description or time.strftime('%m-%d_%H'))
    config = Config(model_name)
    config.batch_size = args.batch_size
    if args.precision:
        config.precision = args.precision
    config.num_epochs = 6 if args.epochs is None else args.epochs
    config.mode = args.dataset
    config.eval_metrics = args.metrics
    config.train_loss = args.loss
    config.logq_correction = not args.no_logq
    if args.data_path:
        config.data_path = os.path.join(args.data_path, '')
    if args.save_path:
        config.save_path = os.path.join(args.save_path, '')
        config.log_path = os.path.join(args.save_path, 'logs', model_name)
    config.__nrms__()

    if args.dataset == 'synthetic':
        config.n_words_title = 30
        corpus = SyntheticMind(config, n_news=4000, seed=0)
        os.makedirs(config.data_path, exist_ok=True)
        emb = os.path.join(config.data_path, config.word_embedding_pretrained)
        if rank == 0 and not os.path.exists(emb):
            np.savez(emb, embeddings=corpus.embedding_table(config.word_embed_size))
        if args.model.lower() == 'nrms_bert':
            # nrms_bert reads one pretrained vector per news id (row r = news id r) from the file beside the word table
            vec = os.path.join(config.data_path, config.bert_embedding_pretrained)
            if rank == 0 and not os.path.exists(vec):
                np.savez(vec, embeddings=corpus.news_vectors(config.bert_embed_size))
        parallel.barrier()
        titles, absts = corpus.id2title_dict, corpus.id2abst_dict
        # (drawn with --negatives epoch too, where nothing trains on them: the dev split below comes from the same generator and
        # stays the one every other run evaluates on)
        train_samples = corpus.train_samples(args.synthetic_users)
        dev_samples, dev_labels = corpus.eval_samples(1024)
        if args.negatives == 'epoch':
            train_imps, train_imp_labels = corpus.train_impressions(args.synthetic_users)
        if args.negatives in ('catalogue', 'adaptive'):
            click_ptr, click_ids = corpus.click_log(args.synthetic_users)
    else:
        if args.dataset == 'demo':
            config.word_embedding_pretrained = 'demo_word_embedding.npz'       # run_demo.py:31
        titles = absts = None                          # MyDataset loads news_title.pkl / news_words.csv itself
        demo = args.dataset == 'demo'
        train_samples = load_dataset(config, 'small_train.pkl' if demo else config.train_data, config.data_path, _type=0)
        dev_samples = load_dataset(config, 'small_dev.pkl' if demo else config.dev_data, config.data_path, _type=1)[:100000]
        dev_labels = read_dev_labels(config)

    recommender = Model(config, args)
    all_train_samples = train_samples
    if world > 1:
        recommender.model._rank_salt = rank * DROPOUT_RANK_SALT
        recommender.model.engine
        parallel.broadcast_parameters(recommender.model._flat)
        # every rank: the same number of equal-sized batches (the gradient all-reduce is collective and the loss is
        # the mean over world * batch_size users): equal shards, incomplete last batches dropped
        per_rank = len(train_samples) // world
        train_samples = train_samples[rank * per_rank:(rank + 1) * per_rank]
    if rank == 0:
        print(model_name, config.device, sum(p.numel() for p in recommender.parameters()), 'parameters')

    def loader(samples, typ, shuffle):
        if args.feed == 'device':
            return DeviceFeed(config, samples, type=typ, id2title_dict=titles, id2abst_dict=absts, batch_size=config.batch_size,
                              device=config.device, shuffle=shuffle, drop_last=(world > 1 and typ == 0), seed=422 + rank)
        return DataLoader(MyDataset(config, samples, type=typ, id2title_dict=titles, id2abst_dict=absts), batch_size=config.batch_size,
                          num_workers=args.num_workers, drop_last=(world > 1 and typ == 0), shuffle=shuffle,
                          pin_memory=True)

    item_window = {}         # item_time / request_time / window_span with --catalogue_window, otherwise no keyword at all
    explain = {} if args.explain is None else {'explain': args.explain}       # otherwise no keyword at all
    item_prior = {}          # item_bias = the click feed's popularity prior with --popularity_prior, otherwise no keyword at all
    click_feed = []          # the ClickFeed of --negatives catalogue / adaptive, once it exists
    item_adjust = {}         # adjust = the click feed's seen-news discount with --seen_discount, otherwise no keyword at all

    def tag_sets(samples, categ):
        # item_tag / allow_tags with --only_categories / --mute_categories, otherwise no keyword at all
        if tag_only is None and tag_mute is None:
            return {}
        n_tags = int(config.category_nums)
        for flag, ids in (('--only_categories', tag_only), ('--mute_categories', tag_mute)):
            if isinstance(ids, tuple) and max(ids) >= n_tags:
                raise SystemExit('%s: category ids must be below %d (got %r)' % (flag, n_tags, ids))
        if not 1 <= n_tags <= 512:
            raise SystemExit('--only_categories / --mute_categories: 1 <= the number of categories <= 512 (got %d)' % n_tags)
        allow = torch.zeros(len(samples), n_tags, dtype=torch.bool)
        if tag_only == 'own':
            if click_feed and samples is click_feed[0][1]:
                # a click log: every category the user clicked in the training part, never the held-out click's
                feed = click_feed[0][0]
                allow = feed.clicked_tags(categ, n_tags)[torch.from_numpy(feed.heldout_users()).to(categ.device)].cpu()
            else:
                for i, smp in enumerate(samples):
                    allow[i, [c for c in smp[1] if 0 <= c < n_tags]] = True
        elif tag_only is not None:
            allow[:, list(tag_only)] = True
        else:
            allow[:] = True
        if tag_mute is not None:
            allow[:, list(tag_mute)] = False
        return {'item_tag': categ, 'allow_tags': allow}

    def tag_words():
        return ', '.join(w for w in ('only ' + ('own' if tag_only == 'own' else ','.join(map(str, tag_only))) if tag_only is not None else '',
                                     'mute ' + ','.join(map(str, tag_mute)) if tag_mute is not None else '') if w)

    def recommend_top(samples):
        # the catalogue is the feed's title table (row r = news id r), so this step always runs on a DeviceFeed
        feed = DeviceFeed(config, samples, type=1, id2title_dict=titles, id2abst_dict=absts, batch_size=config.batch_size,
                          device=config.device)
        if args.recommend_deep is not None:
            return recommend_deep(config, recommender, feed, feed.titles, args.recommend_deep, out_file=args.recommend_out,
                                  **item_prior, **item_window)
        if args.sections is not None:
            info = feed.news_info()
            sections = ((info['categ'], config.category_nums) if args.sections == 'category'
                        else (info['subcateg'], config.subcategory_nums))
            return recommend_sections(config, recommender, feed, feed.titles, args.recommend, sections, out_file=args.recommend_out,
                                      **item_prior)
        if args.combine_filters and args.request_max_per_category is not None:
            n_tags = int(config.category_nums)
            if not 1 <= n_tags <= 512:
                raise SystemExit('--request_max_per_category: 1 <= the number of categories <= 512 (got %d)' % n_tags)
            tags = tag_sets(samples, feed.news_info()['categ'])
            tags.setdefault('item_tag', feed.news_info()['categ'])
            held = {'heldout': [smp[3] for smp in samples]} if click_feed and samples is click_feed[0][1] else {}
            out = recommend_request(config, recommender, feed, feed.titles, args.recommend, out_file=args.recommend_out, **item_prior,
                                    **item_window, **tags, **item_adjust, **held,
                                    tag_caps=torch.full((n_tags,), args.request_max_per_category, dtype=torch.int32))
            st = (recommender.model if hasattr(recommender, 'model') else recommender).last_caps_stats
            print('request with at most {} per category: categories per list: {:.3f}  largest category share: {:.4f}  users: {}{}'.format(
                args.request_max_per_category, st['distinct_tags'], st['largest_share'], st['n_users'],
                ''.join('  hit@{}: {:.4f} +- {:.4f}'.format(kk, st['hit'][kk], st['hit_se'][kk]) for kk in st.get('hit', {}))))
            return out
        if args.combine_filters:
            return recommend_request(config, recommender, feed, feed.titles, args.recommend, out_file=args.recommend_out, **item_prior,
                                     **item_window, **tag_sets(samples, feed.news_info()['categ']), **item_adjust)
        if args.coarse_catalogue:
            out = recommend(config, recommender, feed, feed.titles, args.recommend, out_file=args.recommend_out, coarse=True,
                            coarse_shortlist=args.coarse_shortlist, **explain)
            st = (recommender.model if hasattr(recommender, 'model') else recommender).last_coarse_stats
            print('coarse catalogue: certified share: {:.4f}  users: {}'.format(st['certified'], st['n_users']))
            return out
        if item_adjust:
            out = recommend(config, recommender, feed, feed.titles, args.recommend, out_file=args.recommend_out, **item_prior,
                            **item_adjust)
            # read the file back: how many served news had their user seen (and not clicked) before
            seen_ids = item_adjust['adjust'][0].cpu().numpy()
            filled = served = 0
            with open(out) as f:
                for i, line in enumerate(f):
                    ids = [int(v) for v in line.split(' ', 1)[1].strip()[1:-1].split(',') if v]
                    filled += len(ids)
                    seen = set(seen_ids[i][seen_ids[i] > 0].tolist())
                    served += sum(1 for n in ids if n in seen)
            print('recommend with seen news discounted (beta {:g}, {} slots): {} users, {} of {} slots filled, {} seen news served'.format(
                seen_discount[0], seen_discount[1], len(samples), filled, len(samples) * args.recommend, served))
            return out
        tags = tag_sets(samples, feed.news_info()['categ'])
        if args.max_per_category is not None:
            n_tags = int(config.category_nums)
            if not 1 <= n_tags <= 512:
                raise SystemExit('--max_per_category: 1 <= the number of categories <= 512 (got %d)' % n_tags)
            tags.setdefault('item_tag', feed.news_info()['categ'])
            # the held-out clicks of a click log are at hand: how many of them does the capped list still hold
            held = {'heldout': [smp[3] for smp in samples]} if click_feed and samples is click_feed[0][1] else {}
            net = recommender.model if hasattr(recommender, 'model') else recommender
            out = None
            for name, cap, dst in (('uncapped', args.recommend, os.devnull),
                                   ('at most %d per category' % args.max_per_category, args.max_per_category, args.recommend_out)):
                out = recommend(config, recommender, feed, feed.titles, args.recommend, out_file=dst, **item_prior, **tags, **held,
                                tag_caps=torch.full((n_tags,), cap, dtype=torch.int32))
                st = net.last_caps_stats
                print('{}{}: categories per list: {:.3f}  largest category share: {:.4f}  users: {}{}'.format(
                    name, ' (%s)' % tag_words() if tag_words() else '', st['distinct_tags'], st['largest_share'], st['n_users'],
                    ''.join('  hit@{}: {:.4f} +- {:.4f}'.format(kk, st['hit'][kk], st['hit_se'][kk]) for kk in st.get('hit', {}))))
            return out
        if tags:
            out = recommend(config, recommender, feed, feed.titles, args.recommend, out_file=args.recommend_out, **item_prior, **tags)
            # read the file back: every served id has to carry a category its sample allows
            categ, allow = tags['item_tag'].cpu().numpy(), tags['allow_tags'].numpy()
            filled = outside = 0
            with open(out) as f:
                for i, line in enumerate(f):
                    ids = [int(v) for v in line.split(' ', 1)[1].strip()[1:-1].split(',') if v]
                    filled += len(ids)
                    outside += sum(1 for n in ids if not (0 <= categ[n] < allow.shape[1] and allow[i, categ[n]]))
            print('recommend inside per-user categories ({}): {} users, {} of {} slots filled, {} outside the allowed categories'.format(
                tag_words(), len(samples), filled, len(samples) * args.recommend, outside))
            return out
        if args.diversity is None:
            return recommend(config, recommender, feed, feed.titles, args.recommend, out_file=args.recommend_out, **item_prior,
                             **item_window, **explain)
        # the plain list is the re-ranker's at lambda = 1 (bit for bit), which measures it with the same kernel
        net = recommender.model if hasattr(recommender, 'model') else recommender
        out = None
        for name, lam, dst in (('plain', 1.0, os.devnull), ('diversity %g' % args.diversity, args.diversity, args.recommend_out)):
            out = recommend(config, recommender, feed, feed.titles, args.recommend, out_file=dst, diversity=lam,
                            shortlist=args.shortlist, **item_prior, **item_window, **({} if dst == os.devnull else explain))
            st = net.last_recommend_stats
            print('{}: ILD@{}: {:.4f}  coverage: {:.4f}  users: {}'.format(name, args.recommend, st['ild'], st['coverage'],
                                                                            st['n_users']))
        return out

    def retrieval_quality(samples, labels):
        # as recommend_top: the catalogue is the feed's title table, so always a DeviceFeed
        feed = DeviceFeed(config, samples, type=1, id2title_dict=titles, id2abst_dict=absts, batch_size=config.batch_size,
                          device=config.device)
        net = recommender.model if hasattr(recommender, 'model') else recommender
        needs_info = 'categ' in inspect.signature(net.encode_catalogue).parameters           # nrms_naml's feature rows
        if args.combine_filters:
            return evaluate_retrieval_request(config, recommender, feed, feed.titles, labels, ks=retrieval_ks,
                                              news_info=feed.news_info() if needs_info else None, **item_prior, **item_window,
                                              **tag_sets(samples, feed.news_info()['categ']), **item_adjust)
        return evaluate_retrieval(config, recommender, feed, feed.titles, labels, ks=retrieval_ks,
                                  news_info=feed.news_info() if needs_info else None, **item_prior, **item_window,
                                  **({} if retrieval_nll is None else {'nll_temperatures': retrieval_nll}),
                                  **tag_sets(samples, feed.news_info()['categ']), **item_adjust)

    def attach_graph(feed, samples=None):
        # the click graph is replicated: every rank builds it from ALL training samples (users shard, the graph does not)
        src = feed if samples is None else DeviceFeed(config, samples, type=0, id2title_dict=titles, id2abst_dict=absts,
                                                      batch_size=config.batch_size, device=config.device)
        graph = src.click_graph()
        recommender.model.attach_click_graph(graph, feed.titles)
        if rank == 0:
            print('click graph: {} users, {} news, {} edges, {:.1f} MB in HBM'.format(graph.n_users, graph.n_news, graph.n_edges,
                                                                                    graph.nbytes() / 1e6))

    if not args.test:
        if args.negatives == 'epoch':
            # every rank holds the whole log and draws with the same seed: the negatives of a row do not depend on the rank
            train_feed = ImpressionFeed(config, train_imps, train_imp_labels, id2title_dict=titles, id2abst_dict=absts,
                                        batch_size=config.batch_size, device=config.device, shuffle=True, drop_last=world > 1, seed=422,
                                        rank=rank, world=world)
        elif args.negatives in ('catalogue', 'adaptive'):
            # as above: every rank holds the whole click log and the draw of a click depends on its position in the log only
            # (adaptive: and on the weights, which the ranks share)
            train_feed = ClickFeed(config, click_ptr, click_ids, id2title_dict=titles, id2abst_dict=absts,
                                   news_categ=np.concatenate([[0], corpus.category]), news_subcateg=np.concatenate([[0], corpus.subcategory]),
                                   popularity_power=args.negative_power, batch_size=config.batch_size, device=config.device, shuffle=True,
                                   drop_last=world > 1, seed=422, rank=rank, world=world,
                                   negatives='adaptive' if args.negatives == 'adaptive' else 'popularity',
                                   temperature=args.negative_temperature,
                                   click_time=corpus.click_ticks(click_ptr) if args.catalogue_window is not None else None,
                                   **({} if seen_discount is None else {'seen': corpus.seen_log(click_ptr, click_ids)}))
            if args.negatives == 'adaptive':
                train_feed.attach_scorer(recommender)
            held_samples, held_labels = train_feed.heldout_samples()
            click_feed.append((train_feed, held_samples))
            if seen_discount is not None:
                item_adjust['adjust'] = train_feed.seen_adjustment(seen_discount[0], seen_discount[1], users=train_feed.heldout_users())
            if args.catalogue_window is not None:
                item_window.update(item_time=train_feed.news_first_seen(), request_time=train_feed.heldout_times(),
                                   window_span=args.catalogue_window)
            if args.popularity_prior is not None:
                item_prior['item_bias'] = train_feed.popularity_prior(args.popularity_prior)
        else:
            train_feed = loader(train_samples, 0, True)
        if args.graph == 'global':
            attach_graph(train_feed, all_train_samples if world > 1 and args.negatives != 'epoch' else None)
        hist = train(config, recommender, train_feed, loader(dev_samples, 1, False), dev_labels,
                     max_batches=args.max_batches, verbose=rank == 0)
        if args.graph == 'global' and rank == 0:
            dropped = recommender.model.check_click_graph()
            if dropped:
                print('click graph: {} out-of-batch neighbours dropped (raise config.graph_extra_rows = {})'.format(
                    dropped, config.graph_extra_rows))
        if rank == 0:
            print('final dev AUC:', hist['aucs'][-1] if hist['aucs'] else None)
            if hist['metrics']:
                m = hist['metrics'][-1][1]
                print('final dev AUC: {:.4f}  MRR: {:.4f}  nDCG@5: {:.4f}  nDCG@10: {:.4f}'.format(
                    m['auc'], m['mrr'], m['ndcg5'], m['ndcg10']))
        if args.negatives in ('catalogue', 'adaptive') and rank == 0:
            print('click log: {} rows, {} slots left empty in the last draw'.format(train_feed.n_samples, train_feed.n_short))
        # a click log is evaluated on its own held-out clicks (each user's last one) against the whole catalogue
        top_samples, top_labels = (held_samples, held_labels) if args.negatives in ('catalogue', 'adaptive') else (dev_samples, dev_labels)
        if (args.recommend is not None or args.recommend_deep is not None) and rank == 0:
            print('recommendations saved to', recommend_top(top_samples))
            if args.explain is not None:
                print('reasons saved to', (recommender.model if hasattr(recommender, 'model') else recommender).last_explain_file)
        if retrieval_ks is not None and rank == 0:
            retrieval_quality(top_samples, top_labels)
        return hist
    else:
        # run_v0.py:93-111: the test set through the checkpoint named by --load (or the best one by file-name AUC)
        if args.dataset == 'synthetic':
            test_samples, shown = dev_samples, [len(y) for y in dev_labels]
        else:
            test_samples, shown = load_dataset(config, config.test_data, config.data_path, _type=1), None
        test_feed = loader(test_samples, 1, False)
        if args.graph == 'global':
            # the graph the checkpoint was trained with: the training samples' (all of them, as every training rank builds it)
            attach_graph(test_feed, all_train_samples)
        out = test(config, recommender, test_feed, shown, ckpt_file=args.load,
                   pick_best=args.load is None)
        print('saved to', out)
        if (args.recommend is not None or args.recommend_deep is not None) and rank == 0:
            print('recommendations saved to', recommend_top(test_samples))
            if args.explain is not None:
                print('reasons saved to', (recommender.model if hasattr(recommender, 'model') else recommender).last_explain_file)
        if retrieval_ks is not None and rank == 0:
            retrieval_quality(test_samples, dev_labels)
        return out


if __name__ == '__main__':
    main()
