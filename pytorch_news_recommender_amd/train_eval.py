"""Train / evaluate / test loops with the reference's behaviour
(/root/reference/MIND_2020/train_eval.py:35-153, 219-273, 300-341) on the HIP path.

train():    Adam(lr=config.learning_rate) + CrossEntropy with label 0, loss averaged every 100
            iterations, dev AUC every ``config.eval_step`` batches and at each epoch end, checkpoint
            ``T{time}_{model}_epoch{E}_iter_{n}_auc_{auc:.3f}.ckpt`` when the AUC improves
            (train_eval.py:139-149).  The step itself is ``model.train_step`` (fused HIP forward + CE +
            backward + Adam); ``use_autograd=True`` runs the reference's literal sequence instead
            (``model(batch)`` -> criterion -> backward -> torch.optim.Adam) through the same kernels.
evaluate(): per-impression AUC on the un-padded prefix, unweighted mean (train_eval.py:219-271), with
            the scores never leaving the GPU (``nrms_impression_auc``) instead of a fork pool.
evaluate_metrics(): the same loop scored on AUC, MRR, nDCG@5 and nDCG@10 (``nrms_impression_metrics``).
test():     per-impression rank lists in the MIND submission format (train_eval.py:280-286,335-341), ranked on the
            GPU batch by batch; ``_cal_test`` is the host statement of the same ranks.
recommend(): per impression the k news ids of the WHOLE catalogue the model ranks highest (``model.recommend``, the
            fused top-k kernel nrms_topk_dot), written in test()'s line format.
evaluate_retrieval(): how good those lists are: the exact position of every held-out click in the model's ranking of the
            WHOLE catalogue (``model.rank_targets``, nrms_rank_dot) as Recall@K, MRR, nDCG@K and the median rank.
"""
from __future__ import annotations

import os
import time

import numpy as np
import torch
import torch.nn as nn

from . import parallel


def _inner(model):
    return model.model if hasattr(model, "model") and hasattr(model.model, "train_step") else model


def _pad_labels(y_true, max_c, device):
    n = len(y_true)
    lab = np.zeros((n, max_c), dtype=np.uint8)
    lens = np.zeros(n, dtype=np.int32)
    for i, y in enumerate(y_true):
        k = min(len(y), max_c)
        lab[i, :k] = np.asarray(y[:k], dtype=np.uint8)
        lens[i] = k
    return torch.from_numpy(lab).to(device), torch.from_numpy(lens).to(device)


def _eval_scores(config, model, data_iter, y_true):
    """The scoring loop of evaluate() and evaluate_metrics(): every impression scored in eval mode on the persistent
    news-vector cache, ids checked, the train / eval mode restored.  Returns (net, scores [n, Cmax] device, padded
    labels, lens)."""
    if y_true is None:
        from .data_handler import read_dev_labels
        y_true = read_dev_labels(config)
    net = _inner(model)
    was_training = net.training
    net.eval()
    scores = []
    eng = net.engine
    eng.news_cache_begin()                     # weights are constant from here to the end of the evaluation
    try:
        with torch.no_grad():
            for datas in data_iter:
                scores.append(net(datas))
    finally:
        net.last_eval_cache = eng.news_cache_end()
    net.train(was_training)
    rank_score = torch.cat(scores, dim=0)
    eng.check_ids()
    lab, lens = _pad_labels(y_true[:rank_score.shape[0]], rank_score.shape[1], rank_score.device)
    return net, rank_score, lab, lens


def evaluate(config, model, data_iter, y_true=None, AUC_best=None, verbose=True):
    """y_true: list (one entry per impression, in data_iter order) of 0/1 label lists -- the
    reference keeps it in the module global ``_y_true`` read from dev_behaviors.csv (:36-39); None reads
    that file (data_handler.read_dev_labels).

    Deviation, on purpose: the reference calls ``model.eval()`` here and never ``model.train()`` again (its
    re-enable is commented out, train_eval.py:122,230), so after its first evaluation it trains with dropout
    off.  This evaluate() restores the mode it found."""
    net, rank_score, lab, lens = _eval_scores(config, model, data_iter, y_true)
    aucs = net.engine.impression_auc(rank_score, lab, lens)
    AUC = float(aucs.mean().item())
    net.last_eval_scores, net.last_eval_aucs = rank_score, aucs      # diagnostics (per-impression values of this evaluation)
    if verbose:
        print('AUC:', AUC)
    return AUC


def evaluate_metrics(config, model, data_iter, y_true=None, verbose=True):
    """The four MIND scores of the dev set: dict(auc, mrr, ndcg5, ndcg10), each the unweighted mean over impressions
    (the reference's commented-out lines, train_eval.py:263-270).  Same scoring loop as evaluate(), so ``auc`` is the
    number evaluate() returns on the same weights; the per-impression values come from one nrms_impression_metrics
    pass and are kept in ``last_eval_metrics`` (dict of device tensors: auc, mrr, ndcg@5, ndcg@10).  Tie rule:
    include/nrms_hip.h."""
    net, rank_score, lab, lens = _eval_scores(config, model, data_iter, y_true)
    m = net.engine.impression_metrics(rank_score, lab, lens, ks=(5, 10))
    means = torch.stack([m[k].mean() for k in ("auc", "mrr", "ndcg@5", "ndcg@10")]).cpu().tolist()
    res = dict(zip(("auc", "mrr", "ndcg5", "ndcg10"), means))
    net.last_eval_scores, net.last_eval_aucs, net.last_eval_metrics = rank_score, m["auc"], m
    if verbose:
        print('AUC:', res['auc'])
        print('MRR:', res['mrr'])
        print('nDCG@5:', res['ndcg5'])
        print('nDCG@10:', res['ndcg10'])
    return res


def log_res(config, step, auc):
    if parallel.env_world()[0] != 0:             # one writer: every rank computes the same dev AUC
        return
    os.makedirs(config.log_path, exist_ok=True)
    with open(os.path.join(config.log_path, 'res.txt'), 'a+') as f:
        f.write('{}_{}_:auc_{}\n'.format(time.strftime('%m-%d_%H.%M'), auc, step))


def _save(config, model, total_batch, auc):
    os.makedirs(config.save_path, exist_ok=True)
    name = 'T{}_{}_epoch{}_iter_{}_auc_{:.3f}.ckpt'.format(time.strftime('%m-%d_%H.%M'), config.model_name,
                                                          config.num_epochs, total_batch, auc)
    torch.save(model.state_dict(), os.path.join(config.save_path, name))
    return name


def warmup_lr(base_lr, i, warm_up_steps):
    """Learning rate the reference's warm-up phase applies to iteration ``i`` (0-based): its
    GradualWarmupScheduler(multiplier=1, total_epoch=warm_up_steps) starts at 0 and is stepped with
    ``scheduler.step(i)`` AFTER iteration i (train_eval.py:66-71,99; lr_scheduler.py:41-42), so iteration
    i runs at base_lr * max(i - 1, 0) / warm_up_steps, capped at base_lr."""
    return base_lr * min(max(i - 1, 0) / float(warm_up_steps), 1.0)


def warmup_iterations(warm_up_steps=500):
    """The reference leaves the warm-up loop with ``if i > 500: break`` after running iteration i
    (train_eval.py:97-98): iterations 0..501 whatever warm_up_steps is."""
    return 502


def train(config, model, train_iter, dev_iter=None, dev_labels=None, use_autograd=False, max_batches=None,
          verbose=True):
    """Returns dict(losses=[...per batch...], aucs=[(batch, auc), ...], ckpts=[...], metrics=[(batch, dict), ...]);
    ``metrics`` is filled when config.eval_metrics is set (evaluate_metrics instead of evaluate at every evaluation).
    With config.warm_up the epochs are preceded by the reference's warm-up pass over the first
    batches of train_iter with a linearly increasing learning rate (train_eval.py:64-99)."""
    net = _inner(model)
    if use_autograd and getattr(config, 'train_loss', 'rowwise') == 'pooled':
        raise ValueError("train(use_autograd=True): config.train_loss = 'pooled' exists in the fused train_step only (the criterion of "
                         "the autograd path sees one row of scores per user, not the batch's candidate pool)")
    rank, _, world = parallel.env_world()
    reduce = parallel.GradAllReduce() if world > 1 and torch.distributed.is_initialized() else None
    start = time.time()
    model.train()
    optimizer = criterion = None
    if use_autograd:
        optimizer = torch.optim.Adam(model.parameters(), lr=config.learning_rate)
        criterion = nn.CrossEntropyLoss()
        # this loop zeroes the gradients before every backward and keeps no reference to an old .grad: the backward may
        # hand autograd views of ONE persistent flat buffer instead of 57.6 MB of fresh memory per step (opt-in contract,
        # model/_flat_model.py _FlatFunction.backward)
        net.reuse_grad_buffer = True
    total_batch, AUC_best, STEP_SIZE = 0, 0.56, 100          # train_eval.py:59,61
    hist = dict(losses=[], aucs=[], ckpts=[], warmup_losses=[], metrics=[])

    def dev_auc():
        if not getattr(config, 'eval_metrics', False):
            return evaluate(config, model, dev_iter, dev_labels, AUC_best, verbose)
        m = evaluate_metrics(config, model, dev_iter, dev_labels, verbose)
        hist['metrics'].append((total_batch, m))
        return m['auc']              # checkpoints are still picked by the dev AUC alone

    window = []
    done = False
    if getattr(config, 'warm_up', False):
        if verbose:
            print('warm-up training...')
        wlosses = []
        for i, datas in enumerate(train_iter):
            lr_i = warmup_lr(config.learning_rate, i, config.warm_up_steps)
            if use_autograd:
                for grp in optimizer.param_groups:
                    grp['lr'] = lr_i
                outputs = model(datas)
                model.zero_grad()
                loss = criterion(outputs, torch.zeros(len(outputs), dtype=torch.long, device=outputs.device))
                loss.backward()
                optimizer.step()
                wlosses.append(loss.detach())
            else:
                wlosses.append(net.train_step(datas, lr=lr_i, world_size=world, all_reduce=reduce) /
                               len(datas['browsed_titles']))
            if i % 100 == 0 and verbose:
                print('Warm-up Steps: {0:>6},  Train Loss: {1:>5.6}'.format(i, float(wlosses[-1])))
            if i + 1 >= warmup_iterations(config.warm_up_steps) or (max_batches is not None and i + 1 >= max_batches):
                break
        hist['warmup_losses'] = [float(v) for v in wlosses]
        if use_autograd:
            for grp in optimizer.param_groups:
                grp['lr'] = config.learning_rate
    for epoch in range(config.num_epochs):
        if verbose:
            print('Epoch [{}/{}]'.format(epoch + 1, config.num_epochs))
        if hasattr(net, 'refresh_neighbor_vectors'):
            # graph model with an attached click graph: out-of-batch neighbour vectors are at most one epoch stale
            # (model/graph_hip.py, staleness rule); a no-op otherwise
            net.refresh_neighbor_vectors()
        for datas in train_iter:
            B = len(datas['browsed_titles'])
            if use_autograd:
                outputs = model(datas)
                model.zero_grad()
                y = torch.zeros(len(outputs), dtype=torch.long, device=outputs.device)
                loss = criterion(outputs, y)
                loss.backward()
                optimizer.step()
                window.append(loss.detach())
            else:
                loss_sum = net.train_step(datas, world_size=world, all_reduce=reduce)
                window.append(loss_sum / B)
            if total_batch % STEP_SIZE == 0:                 # one host sync per 100 iterations, not two per step
                vals = [float(v) for v in window]
                # out-of-range word ids surface here: after the very first batch (total_batch == 0: a vocabulary / table
                # mismatch is caught before a second update is applied, where nn.Embedding would have raised) and then
                # every 100 steps
                net.engine.check_ids()
                hist['losses'].extend(vals)
                window = []
                if verbose:
                    print('Iter: {0:>6},  Train Loss: {1:>5.6},  Time: {2:.1f}s'.format(
                        total_batch, float(np.mean(vals)), time.time() - start))
            total_batch += 1
            if dev_iter is not None and total_batch % config.eval_step == 0:
                auc = dev_auc()
                hist['aucs'].append((total_batch, auc))
                log_res(config, auc, total_batch)
                if auc > AUC_best:
                    AUC_best = auc
                    if config.save_flag and rank == 0:
                        hist['ckpts'].append(_save(config, model, total_batch, AUC_best))
            if max_batches is not None and total_batch >= max_batches:
                done = True
                break
        if dev_iter is not None:
            auc = dev_auc()
            hist['aucs'].append((total_batch, auc))
            log_res(config, auc, 'epoch_{}'.format(epoch))
            if auc > AUC_best:
                AUC_best = auc
                if config.save_flag and rank == 0:
                    hist['ckpts'].append(_save(config, model, total_batch, AUC_best))
        if done:
            break
    hist['losses'].extend(float(v) for v in window)
    return hist


def _cal_test(scores, n):
    """Rank (1 = best) of each shown candidate (train_eval.py:280-286).  Host reference of the submission ranks that
    test() computes on the GPU (nrms_impression_metrics)."""
    res = np.argsort(-np.asarray(scores[:n]), kind="stable")
    rank = [0] * n
    for pos, v in enumerate(res):
        rank[v] = pos + 1
    return rank


def best_checkpoint(config):
    """The checkpoint of this model name with the highest dev AUC in its file name
    (``..._auc_0.673.ckpt``, written by train(); selection rule of train_eval.py:303-308, parsed as a float
    instead of ``eval``).  None if there is none above 0.5."""
    best, best_auc = None, 0.5
    if not os.path.isdir(config.save_path):
        return None
    for ckpt in sorted(os.listdir(config.save_path)):
        if config.model_name not in ckpt or not ckpt.endswith('.ckpt'):
            continue
        try:
            auc = float(ckpt[:-len('.ckpt')].split('_')[-1])
        except ValueError:
            continue
        if auc > best_auc:
            best, best_auc = ckpt, auc
    return best


def test(config, model, data_iter, test_list_nums=None, ckpt_file=None, out_file=None, pick_best=False):
    """Writes ``<impression index> [r1,r2,...]`` lines; returns the file name.  test_list_nums: shown
    candidates per impression (None: data_handler.get_Test_List, train_eval.py:287-298,315); pick_best: load the
    best checkpoint by file-name AUC when ckpt_file is None (train_eval.py:301-310)."""
    net = _inner(model)
    if ckpt_file is None and pick_best:
        ckpt_file = best_checkpoint(config)
        if ckpt_file is None:
            # the reference fails here too (it loads './save_model/' + None, train_eval.py:309): scoring whatever weights
            # the model happens to hold and writing a submission from them would be a silent wrong answer
            raise FileNotFoundError("test(pick_best=True): no checkpoint of model %r with a dev AUC above 0.5 in %r"
                                    % (config.model_name, config.save_path))
    if ckpt_file is not None:
        print('loading checkpoint:', os.path.join(config.save_path, ckpt_file))
        model.load_state_dict(torch.load(os.path.join(config.save_path, ckpt_file), weights_only=True))
    if test_list_nums is None:
        from .data_handler import get_Test_List
        test_list_nums = get_Test_List(config)
    net.eval()
    eng = net.engine
    ranks = []
    eng.news_cache_begin()
    try:
        with torch.no_grad():
            for datas in data_iter:
                # each batch ranked on the GPU (nrms_impression_metrics, the tie rule of _cal_test); only int32 ranks come back
                s = net(datas)
                nums = [int(n) for n in test_list_nums[len(ranks):len(ranks) + s.shape[0]]]
                if not nums:
                    continue
                s = s[:len(nums)]
                lens = torch.tensor(nums, dtype=torch.int32).to(s.device)
                lab = torch.zeros(s.shape, dtype=torch.uint8, device=s.device)
                rk = eng.impression_metrics(s, lab, lens, ranks=True)["ranks"].cpu().numpy()
                # a row shorter than its shown count keeps _cal_test's trailing zeros
                ranks.extend(rk[i, :n].tolist() + [0] * (n - rk.shape[1]) for i, n in enumerate(nums))
    finally:
        eng.news_cache_end()
    eng.check_ids()
    file_name = out_file or 'sumbit_{}_{}.txt'.format(config.model_name, time.strftime('%m-%d_%H.%M', time.localtime()))
    with open(file_name, 'w') as f:
        for i, r in enumerate(ranks):
            f.write(str(i + 1) + ' ')
            f.write(str(r).replace(' ', '') + '\n')
    return file_name


class _TagSets:
    """The tag keywords of recommend() / evaluate_retrieval(), turned into ``model.recommend_tagged`` / ``rank_targets_tagged``
    arguments batch by batch: item_tag int [N] by news id on the model's device, allow_tags bool [n_samples, n_tags] (numpy or
    torch), one row per sample of data_iter in its order.  Both or neither (ValueError); with tags, the keywords of ``refused``
    that were given raise a ValueError that names them: the tagged kernels have no time window, cursor, fp16 shortlist, diversity
    re-ranking, log-partition or attribution form."""

    def __init__(self, who, item_tag, allow_tags, refused):
        self.on = item_tag is not None and allow_tags is not None
        if (item_tag is None) != (allow_tags is None):
            raise ValueError("%s: item_tag and allow_tags go together (item_tag %s, allow_tags %s)"
                             % (who, "missing" if item_tag is None else "given", "missing" if allow_tags is None else "given"))
        if not self.on:
            return
        for name, given in refused:
            if given:
                raise ValueError("%s: %s does not go with item_tag / allow_tags: the tagged calls serve and rank the plain or "
                                 "the biased list only" % (who, name))
        self.who, self.item_tag = who, item_tag
        self.allow = torch.as_tensor(allow_tags)
        if self.allow.dim() != 2 or self.allow.dtype != torch.bool:
            raise ValueError("%s: allow_tags must be bool [n_samples, n_tags] (got %s %s)"
                             % (who, tuple(self.allow.shape), self.allow.dtype))

    def of(self, done, B, dev):
        if done + B > self.allow.shape[0]:
            raise ValueError("%s: %d allow_tags rows for %d samples" % (self.who, self.allow.shape[0], done + B))
        return self.item_tag, self.allow[done:done + B].to(dev)


class _TagCaps:
    """The cap keywords of recommend(), turned into ``model.recommend_capped`` arguments batch by batch.  tag_caps: an int tensor
    or array [n_tags] (every sample) or [n_samples, n_tags] (one row per sample of data_iter in its order), or an int when
    allow_tags gives n_tags; item_tag as for the tag sets (required); allow_tags optional, bool [n_samples, n_tags]: a closed tag
    becomes cap 0.  heldout optional: per sample the news ids of its held-out clicks (a list of lists, or an int tensor
    [n_samples] / [n_samples, T] with -1 for none).  With caps, the keywords of ``refused`` that were given raise a ValueError that
    names them."""

    def __init__(self, who, tag_caps, item_tag, allow_tags, heldout, refused):
        self.on = tag_caps is not None
        if not self.on:
            if heldout is not None:
                raise ValueError("%s: heldout is read with tag_caps only (give tag_caps)" % who)
            return
        if item_tag is None:
            raise ValueError("%s: tag_caps caps the tags of item_tag (give item_tag)" % who)
        for name, given in refused:
            if given:
                raise ValueError("%s: %s does not go with tag_caps: the capped call serves the plain or the biased list only"
                                 % (who, name))
        self.who, self.item_tag = who, item_tag
        self.allow = None
        if allow_tags is not None:
            self.allow = torch.as_tensor(allow_tags)
            if self.allow.dim() != 2 or self.allow.dtype != torch.bool:
                raise ValueError("%s: allow_tags must be bool [n_samples, n_tags] (got %s %s)"
                                 % (who, tuple(self.allow.shape), self.allow.dtype))
        caps = torch.as_tensor(tag_caps)
        if caps.dtype not in (torch.int32, torch.int64) or caps.dim() > 2:
            raise ValueError("%s: tag_caps must be an int, or an int tensor [n_tags] or [n_samples, n_tags] (got %s %s)"
                             % (who, tuple(caps.shape), caps.dtype))
        if caps.dim() == 0:
            if self.allow is None:
                raise ValueError("%s: an int tag_caps needs allow_tags to say how many tags there are (or give an [n_tags] tensor)" % who)
            caps = caps.expand(self.allow.shape[1])
        if self.allow is not None and self.allow.shape[1] != caps.shape[-1]:
            raise ValueError("%s: tag_caps %s and allow_tags %s disagree on n_tags" % (who, tuple(caps.shape), tuple(self.allow.shape)))
        self.caps = caps.clamp(0, 2 ** 31 - 1).to(torch.int32)
        self.n_tags = int(caps.shape[-1])
        self.held = None
        if heldout is not None:
            if torch.is_tensor(heldout) or isinstance(heldout, np.ndarray):
                held = torch.as_tensor(heldout).to(torch.int64)
                self.held = held.view(-1, 1) if held.dim() == 1 else held
            else:
                T = max([len(h) for h in heldout] + [1])
                self.held = torch.tensor([list(h) + [-1] * (T - len(h)) for h in heldout], dtype=torch.int64).view(len(heldout), T)
        self.sums = None          # on the device: lists, distinct tags, largest shares, held-out clicks, hits at every K'

    def of(self, done, B, dev):
        """-> (item_tag, cap int32 [B, n_tags] on dev) for samples [done, done + B)."""
        for name, t in (("tag_caps", self.caps if self.caps.dim() == 2 else None), ("allow_tags", self.allow), ("heldout", self.held)):
            if t is not None and done + B > t.shape[0]:
                raise ValueError("%s: %d %s rows for %d samples" % (self.who, t.shape[0], name, done + B))
        cap = (self.caps[done:done + B] if self.caps.dim() == 2 else self.caps.unsqueeze(0).expand(B, -1)).to(dev)
        if self.allow is not None:
            cap = torch.where(self.allow[done:done + B].to(dev), cap, torch.zeros_like(cap))
        return self.item_tag, cap.contiguous()

    def note(self, done, ids, ks):
        """Accumulates the statistics of one batch's ids [B, k] (news ids, -1 padding) on their device, with torch alone."""
        dev, n_tags = ids.device, self.n_tags
        tag = self.item_tag.to(dev, dtype=torch.int64)[ids.clamp(min=0)]
        ok = (ids >= 0) & (tag >= 0) & (tag < n_tags)
        count = torch.zeros(ids.shape[0], n_tags + 1, dtype=torch.int64, device=dev)
        count.scatter_add_(1, torch.where(ok, tag, torch.full_like(tag, n_tags)), torch.ones_like(tag))
        count = count[:, :n_tags]
        n = ok.sum(dim=1)
        some = n > 0
        share = count.max(dim=1).values.double() / n.clamp(min=1).double()
        vals = [some.sum().double(), ((count > 0).sum(dim=1) * some).sum().double(), (share * some).sum()]
        if self.held is not None:
            held = self.held[done:done + ids.shape[0]].to(dev)
            vals.append((held >= 1).sum().double())
            for kk in ks:          # plain list membership: is the held-out click among the first kk of its sample's list
                hit = (held.unsqueeze(2) == ids[:, :kk].unsqueeze(1)).any(dim=2) & (held >= 1)
                vals.append(hit.sum().double())
        vals = torch.stack(vals)
        self.sums = vals if self.sums is None else self.sums + vals

    def stats(self, ks):
        """The run's statistics (one host synchronisation): the mean number of distinct tags per non-empty list, the mean largest
        share of one tag in such a list, and, with heldout, per K' the share of held-out clicks found among the first K' of their
        sample's list with its binomial standard error."""
        v = self.sums.cpu().tolist() if self.sums is not None else [0.0] * (3 + (0 if self.held is None else 1 + len(ks)))
        n = int(v[0])
        res = {"distinct_tags": v[1] / n if n else float("nan"), "largest_share": v[2] / n if n else float("nan"), "n_users": n}
        if self.held is not None:
            m = int(v[3])
            res["n_heldout"] = m
            res["hit"] = {kk: (h / m if m else float("nan")) for kk, h in zip(ks, v[4:])}
            res["hit_se"] = {kk: ((p * (1.0 - p) / m) ** 0.5 if m else float("nan")) for kk, p in res["hit"].items()}
        return res


class _Adjust:
    """The ``adjust`` keyword of recommend() / evaluate_retrieval(), turned into ``model.recommend_adjusted`` /
    ``rank_targets_adjusted`` arguments batch by batch: adjust = (news_ids int [n_samples, E], delta float [n_samples, E]) (numpy or
    torch; ``data_handler.seen_adjustment``), one row per sample of data_iter in its order, E <= 256.  With it, the keywords of
    ``refused`` that were given raise a ValueError that names them: the adjusted kernels have no time window, tag set, caps, fp16
    shortlist, diversity re-ranking, log-partition or attribution form."""

    def __init__(self, who, adjust, refused):
        self.on = adjust is not None
        if not self.on:
            return
        for name, given in refused:
            if given:
                raise ValueError("%s: %s does not go with adjust: the adjusted calls serve and rank the plain or the biased list "
                                 "only" % (who, name))
        if not isinstance(adjust, (tuple, list)) or len(adjust) != 2:
            raise ValueError("%s: adjust must be a pair (news_ids [n_samples, E], delta [n_samples, E]) (got %s)"
                             % (who, type(adjust).__name__))
        self.who = who
        self.ids, self.delta = torch.as_tensor(adjust[0]), torch.as_tensor(adjust[1])
        if (self.ids.dim() != 2 or self.ids.shape != self.delta.shape or self.ids.dtype not in (torch.int32, torch.int64)
                or not self.delta.dtype.is_floating_point or self.ids.shape[1] > 256):
            raise ValueError("%s: adjust must be (int news_ids [n_samples, E], float delta [n_samples, E]) of one shape, E <= 256 "
                             "(got %s %s and %s %s)" % (who, tuple(self.ids.shape), self.ids.dtype, tuple(self.delta.shape),
                                                        self.delta.dtype))

    def of(self, done, B, dev):
        if done + B > self.ids.shape[0]:
            raise ValueError("%s: %d adjust rows for %d samples" % (self.who, self.ids.shape[0], done + B))
        return (self.ids[done:done + B].to(dev, dtype=torch.int64), self.delta[done:done + B].to(dev, dtype=torch.float32))


class _RequestWindows:
    """The time-window keywords of recommend() / evaluate_retrieval(), turned into ``model.recommend`` / ``rank_targets`` keywords
    batch by batch: sample i is served inside [request_time[i] - window_span, request_time[i] + 1), clamped to int32.  All three or
    none (ValueError); with none, ``of`` returns {} and the model is called exactly as before."""

    def __init__(self, who, item_time, request_time, window_span):
        given = [item_time is not None, request_time is not None, window_span is not None]
        self.on = all(given)
        if any(given) and not self.on:
            raise ValueError("%s: item_time, request_time and window_span go together" % who)
        if not self.on:
            return
        span = int(window_span)
        if span < 1:
            raise ValueError("%s: window_span must be >= 1 (got %r)" % (who, window_span))
        rt = np.asarray(request_time, dtype=np.int64).reshape(-1)
        lo, hi = np.iinfo(np.int32).min, np.iinfo(np.int32).max
        self.who, self.item_time = who, item_time
        self.window = np.stack([np.clip(rt - span, lo, hi), np.clip(rt + 1, lo, hi)], axis=1).astype(np.int32)

    def of(self, done, B, dev):
        if not self.on:
            return {}
        if done + B > len(self.window):
            raise ValueError("%s: %d request times for %d samples" % (self.who, len(self.window), done + B))
        return {"item_time": self.item_time, "window": torch.from_numpy(self.window[done:done + B]).to(dev)}


def recommend(config, model, data_iter, titles, k, out_file=None, exclude_history=True, news_info=None, diversity=None,
              shortlist=None, item_bias=None, item_time=None, request_time=None, window_span=None, coarse=False,
              coarse_shortlist=None, adjust=None, tag_caps=None, heldout=None, item_tag=None, allow_tags=None, explain=None):
    """Writes ``<impression index> [id1,id2,...]`` lines (1-based, as test()): per impression of data_iter the k news ids
    of the whole catalogue the model recommends, best first.  titles: [N, L] word ids with row r = news id r
    (``DeviceFeed.titles``); it is encoded once.  news_info: the per-news tables nrms_naml and hierec need
    (``DeviceFeed.news_info()``), passed to encode_catalogue as keyword arguments.  With exclude_history the user's
    browsed news are left out.  Should the catalogue hold fewer than k eligible news for a user, the line is shorter.
    Returns the file name.

    diversity / shortlist: ``model.recommend``'s re-ranking by maximal marginal relevance (the file format is the same, the
    lines are in pick order).  With ``diversity`` given (models that re-rank) the call leaves
    ``net.last_recommend_stats = {"ild": mean intra-list diversity over the users with at least two news, "coverage":
    distinct recommended news / (N - 1), "n_users": those users}`` (NaN / 0 without such users), with one host
    synchronisation at the end; without it the attribute is set to None and the model is called exactly as before.

    item_bias: ``model.recommend``'s per-news prior (float32 [N] by news id on the model's device, e.g.
    ``ClickFeed.popularity_prior(alpha)``), with or without ``diversity``.  None: the keyword is not passed at all.

    item_time / request_time / window_span (all three or none): a time window of the catalogue per sample.  item_time: int [N]
    by news id on the model's device (``ClickFeed.news_first_seen()``); request_time: one tick per sample of data_iter, in its
    order; sample i only gets news with request_time[i] - window_span <= item_time[id] <= request_time[i]
    (``model.recommend(item_time=..., window=...)``).  None: the keywords are not passed at all.

    coarse / coarse_shortlist: serve through ``model.recommend(coarse=...)``, the fp16 shortlist with a certificate: the catalogue
    is packed once after it is encoded (``model.pack_catalogue``), the file is the same, bit for bit, and the call leaves
    ``net.last_coarse_stats = {"certified": share of the users whose row the certificate covered, "n_users": users}`` (None
    without ``coarse``, when the model is called exactly as before).  Not with diversity, item_bias or a time window (ValueError).

    item_tag / allow_tags (both or neither): a set of news tags per sample, ``model.recommend_tagged``.  item_tag: int [N] by news
    id on the model's device (``DeviceFeed.news_info()["categ"]``); allow_tags: bool [n_samples, n_tags], one row per sample of
    data_iter in its order (``ClickFeed.clicked_tags``): sample i only gets news whose tag it allows.  With or without item_bias;
    not with diversity, coarse, a time window or explain (ValueError naming the keyword).  None: the model is called exactly as
    before.

    tag_caps (with item_tag; allow_tags optional): a hard cap per news tag, ``model.recommend_capped``.  tag_caps: an int tensor
    [n_tags] (the same caps for every sample) or [n_samples, n_tags], or an int when allow_tags says how many tags there are:
    sample i's list holds at most tag_caps[i, t] news of tag t (the exact ranking walked greedily); with allow_tags as well a closed
    tag becomes cap 0.  With or without item_bias; not with diversity, coarse, a time window or explain (ValueError naming the
    keyword).  The call leaves ``net.last_caps_stats = {"distinct_tags": mean number of distinct tags per non-empty list,
    "largest_share": mean over those lists of the largest share one tag holds, "n_users": those lists}``, computed with torch on
    the returned ids, with one host synchronisation at the end.  heldout (with tag_caps only): per sample the news ids of its
    held-out clicks (a list of lists, or an int tensor with -1 for none); the stats gain ``"hit": {K': share of the held-out clicks
    found among the first K' of their sample's list}`` for K' in (1, 5, 10, 20, 50, 100, k) up to k, ``"hit_se"`` (the binomial
    standard error) and ``"n_heldout"``: plain list membership, no rank kernel.  None: the model is called exactly as before and
    ``last_caps_stats`` is None.

    explain = m in [1, 8]: also writes ``<file name>.reasons`` and leaves its name in ``net.last_explain_file`` (None without
    ``explain``, when the model is called and the list is written exactly as before; the list file is the same either way).  One
    line per recommended news, in the order of the list file:
    ``<impression index> <news id> <total> <padding share> [<browsed id>:<contribution>,...]``: ``model.explain`` of the ids every
    path above ends with (so it goes with diversity, item_bias, a time window and coarse): the score without any item_bias, the
    part of it carried by the history's padding slots, and the up to m clicks of the history with the largest contributions,
    largest first, negative ones included.  Numbers are written with 9 significant digits, which names every float32: two runs
    give the same bytes.  Needs a model with ``CATALOGUE_EXPLAIN`` (ValueError otherwise, before anything is encoded).

    adjust = (news_ids [n_samples, E], delta [n_samples, E]): per-sample score adjustments, ``model.recommend_adjusted``
    (``data_handler.seen_adjustment`` builds the seen-news discount): sample i's score of news news_ids[i, e] moves by delta[i, e];
    id 0 is an empty slot.  One row per sample of data_iter in its order, sliced per batch.  With or without item_bias; not with
    diversity, coarse, a time window, item_tag / allow_tags, tag_caps or explain (ValueError naming the keyword).  None: no new
    keyword reaches the model, which is called exactly as before."""
    net = _inner(model)
    adj = _Adjust("recommend", adjust, (("diversity", diversity is not None or shortlist is not None),
                                        ("coarse", bool(coarse) or coarse_shortlist is not None),
                                        ("item_time / request_time / window_span", item_time is not None or request_time is not None
                                         or window_span is not None),
                                        ("tag_caps", tag_caps is not None or heldout is not None),
                                        ("item_tag / allow_tags", item_tag is not None or allow_tags is not None),
                                        ("explain", explain is not None)))
    caps = _TagCaps("recommend", tag_caps, item_tag, allow_tags, heldout,
                    (("diversity", diversity is not None or shortlist is not None),
                     ("coarse", bool(coarse) or coarse_shortlist is not None),
                     ("item_time / request_time / window_span", item_time is not None or request_time is not None
                      or window_span is not None), ("explain", explain is not None)))
    if caps.on:
        item_tag = allow_tags = None          # the caps carry them; the tag sets below stay off
    tags = _TagSets("recommend", item_tag, allow_tags, (("diversity", diversity is not None or shortlist is not None),
                                                        ("coarse", bool(coarse) or coarse_shortlist is not None),
                                                        ("item_time / request_time / window_span", item_time is not None
                                                         or request_time is not None or window_span is not None),
                                                        ("explain", explain is not None)))
    if explain is not None:
        if not getattr(net, "CATALOGUE_EXPLAIN", False):
            raise ValueError("recommend: explain needs a model whose score is one additive-attention sum over the clicks of the "
                             "history (model.explain; CATALOGUE_EXPLAIN)")
        if not 1 <= int(explain) <= 8:
            raise ValueError("recommend: explain = m must be in [1, 8] (got %r)" % (explain,))
    reasons = []

    def note(datas, ids):
        if explain is not None:
            reasons.append([t.cpu() for t in (ids,) + tuple(net.explain(datas, ids, catalogue, int(explain))[:4])])

    prior = {} if item_bias is None else {"item_bias": item_bias}
    windows, done = _RequestWindows("recommend", item_time, request_time, window_span), 0
    if diversity is None and shortlist is not None:
        raise ValueError("recommend: shortlist is the candidate count of the diversity re-ranking (give diversity)")
    if coarse_shortlist is not None and not coarse:
        raise ValueError("recommend: coarse_shortlist is the shortlist length of the fp16 shortlist path (give coarse=True)")
    if coarse and (diversity is not None or item_bias is not None or windows.on):
        raise ValueError("recommend: coarse serves the plain list only (no diversity, item_bias or time window)")
    catalogue = net.encode_catalogue(titles, **(news_info or {}))
    lines = []
    net.last_coarse_stats = None
    if coarse:
        packed = net.pack_catalogue(catalogue)
        net.last_recommend_stats = None
        n_cert = torch.zeros((), dtype=torch.int64, device=catalogue.device)
        n_users = 0
        for datas in data_iter:
            ids, _, cert = net.recommend(datas, k, catalogue, exclude_history=exclude_history, coarse=packed,
                                         coarse_shortlist=coarse_shortlist, return_certified=True)
            n_cert += cert.sum()
            n_users += int(cert.shape[0])
            lines.extend(ids.cpu().tolist())
            note(datas, ids)
        net.last_coarse_stats = {"certified": int(n_cert.item()) / n_users if n_users else float("nan"), "n_users": n_users}
    elif caps.on:
        net.last_recommend_stats = None
        hit_ks = tuple(kk for kk in (1, 5, 10, 20, 50, 100) if kk < int(k)) + (int(k),)
        for datas in data_iter:
            B = int(torch.as_tensor(datas["browsed_ids"]).shape[0])
            tag, cap = caps.of(done, B, catalogue.device)
            ids, _ = net.recommend_capped(datas, k, catalogue, tag, cap, exclude_history=exclude_history, **prior)
            caps.note(done, ids, hit_ks)
            done += B
            lines.extend(ids.cpu().tolist())
    elif tags.on:
        net.last_recommend_stats = None
        for datas in data_iter:
            B = int(torch.as_tensor(datas["browsed_ids"]).shape[0])
            tag, allow = tags.of(done, B, catalogue.device)
            done += B
            ids, _ = net.recommend_tagged(datas, k, catalogue, tag, allow, exclude_history=exclude_history, **prior)
            lines.extend(ids.cpu().tolist())
    elif adj.on:
        net.last_recommend_stats = None
        for datas in data_iter:
            B = int(torch.as_tensor(datas["browsed_ids"]).shape[0])
            slots = adj.of(done, B, catalogue.device)
            done += B
            ids, _ = net.recommend_adjusted(datas, k, catalogue, slots, exclude_history=exclude_history, **prior)
            lines.extend(ids.cpu().tolist())
    elif diversity is None:
        net.last_recommend_stats = None
        for datas in data_iter:
            if windows.on:
                B = int(torch.as_tensor(datas["browsed_ids"]).shape[0])
                prior.update(windows.of(done, B, catalogue.device))
                done += B
            ids, _ = net.recommend(datas, k, catalogue, exclude_history=exclude_history, **prior)
            lines.extend(ids.cpu().tolist())
            note(datas, ids)
    else:
        rows, ilds = [], []
        for datas in data_iter:
            if windows.on:
                B = int(torch.as_tensor(datas["browsed_ids"]).shape[0])
                prior.update(windows.of(done, B, catalogue.device))
                done += B
            ids, _, ild = net.recommend(datas, k, catalogue, exclude_history=exclude_history, diversity=diversity,
                                        shortlist=shortlist, return_ild=True, **prior)
            rows.append(ids)
            ilds.append(ild)
            note(datas, ids)
        n_news = int(catalogue.shape[0])
        dev = catalogue.device
        ids = torch.cat(rows) if rows else torch.zeros(0, int(k), dtype=torch.int64, device=dev)
        ild = torch.cat(ilds).double() if ilds else torch.zeros(0, dtype=torch.float64, device=dev)
        seen = torch.zeros(n_news + 1, dtype=torch.bool, device=dev)           # slot n_news takes the -1 padding
        seen[torch.where(ids >= 0, ids, torch.full_like(ids, n_news)).reshape(-1)] = True
        have = ~torch.isnan(ild)
        stats = torch.stack([torch.where(have, ild, torch.zeros_like(ild)).sum() / have.sum().clamp(min=1),
                             seen[1:n_news].sum().double() / max(1, n_news - 1), have.sum().double()]).cpu().tolist()
        n_users = int(stats[2])                                                # (the one host synchronisation is above)
        net.last_recommend_stats = {"ild": stats[0] if n_users else float("nan"), "coverage": stats[1], "n_users": n_users}
        lines = ids.cpu().tolist()
    net.last_caps_stats = caps.stats(hit_ks) if caps.on else None
    net.engine.check_ids()
    net.check_recommend_ids()
    file_name = out_file or 'recommend_{}_{}.txt'.format(config.model_name, time.strftime('%m-%d_%H.%M', time.localtime()))
    with open(file_name, 'w') as f:
        for i, row in enumerate(lines):
            f.write(str(i + 1) + ' ')
            f.write(str([n for n in row if n >= 0]).replace(' ', '') + '\n')
    net.last_explain_file = None
    if explain is not None:
        net.last_explain_file = file_name + '.reasons'
        with open(net.last_explain_file, 'w') as f:
            i = 0
            for ids, r_ids, r_contrib, total, pad in reasons:
                for b in range(ids.shape[0]):
                    i += 1
                    for j, n in enumerate(ids[b].tolist()):
                        if n < 0:
                            continue
                        why = ','.join('%d:%.9g' % (r, c) for r, c in zip(r_ids[b, j].tolist(), r_contrib[b, j].tolist()) if r >= 0)
                        f.write('%d %d %.9g %.9g [%s]\n' % (i, n, float(total[b, j]), float(pad[b, j]), why))
    return file_name


def recommend_deep(config, model, data_iter, titles, K, out_file=None, exclude_history=True, news_info=None, item_bias=None,
                   item_time=None, request_time=None, window_span=None):
    """recommend() at a depth of up to 4096 (candidates for a re-ranker): writes the same ``<impression index> [id1,id2,...]``
    lines, per impression of data_iter the first K news ids of the model's ranking of the whole catalogue, best first
    (``model.recommend_deep``: pages of 256 chained on the device).  titles / news_info / exclude_history / item_bias / item_time /
    request_time / window_span as in recommend(); there is no diversity re-ranking and no fp16 shortlist at this depth.  Returns
    the file name."""
    net = _inner(model)
    prior = {} if item_bias is None else {"item_bias": item_bias}
    windows, done = _RequestWindows("recommend_deep", item_time, request_time, window_span), 0
    K = int(K)
    if not 1 <= K <= 4096:
        raise ValueError("recommend_deep: K must be in [1, 4096] (got %d)" % K)
    catalogue = net.encode_catalogue(titles, **(news_info or {}))
    lines = []
    for datas in data_iter:
        if windows.on:
            B = int(torch.as_tensor(datas["browsed_ids"]).shape[0])
            prior.update(windows.of(done, B, catalogue.device))
            done += B
        ids, _ = net.recommend_deep(datas, K, catalogue, exclude_history=exclude_history, **prior)
        lines.extend(ids.cpu().tolist())
    net.engine.check_ids()
    net.check_recommend_ids()
    file_name = out_file or 'recommend_{}_{}.txt'.format(config.model_name, time.strftime('%m-%d_%H.%M', time.localtime()))
    with open(file_name, 'w') as f:
        for i, row in enumerate(lines):
            f.write(str(i + 1) + ' ')
            f.write(str([n for n in row if n >= 0]).replace(' ', '') + '\n')
    return file_name


def recommend_sections(config, model, data_iter, titles, k, sections, out_file=None, exclude_history=True, news_info=None,
                       item_bias=None):
    """The front page by section: writes ``<impression index> <section> [id1,id2,...]`` lines (the index 1-based, as
    recommend()): per impression of data_iter and per section the k news ids of that section the model recommends, best
    first (``model.recommend_sections``).  sections: (section_of, n_sections), the section of every news id (int64 [N], e.g.
    ``DeviceFeed.news_info()["categ"]``) and their count.  titles / news_info / exclude_history / item_bias as in
    recommend(); the catalogue is encoded and sectioned once.  A section that holds no eligible news for a user is skipped,
    one with fewer than k gives a shorter line.  Returns the file name."""
    net = _inner(model)
    prior = {} if item_bias is None else {"item_bias": item_bias}
    section_of, n_sections = sections
    sectioned = net.section_catalogue(net.encode_catalogue(titles, **(news_info or {})), section_of, n_sections)
    rows = []
    for datas in data_iter:
        ids, _ = net.recommend_sections(datas, k, sectioned, exclude_history=exclude_history, **prior)
        rows.extend(ids.cpu().tolist())
    net.engine.check_ids()
    net.check_recommend_ids()
    file_name = out_file or 'recommend_sections_{}_{}.txt'.format(config.model_name, time.strftime('%m-%d_%H.%M', time.localtime()))
    with open(file_name, 'w') as f:
        for i, per_section in enumerate(rows):
            for g, row in enumerate(per_section):
                got = [n for n in row if n >= 0]
                if got:
                    f.write('%d %d %s\n' % (i + 1, g, str(got).replace(' ', '')))
    return file_name


def evaluate_retrieval(config, model, data_iter, titles, y_true, ks=(10, 100), exclude_history=True, news_info=None,
                       verbose=True, item_bias=None, item_time=None, request_time=None, window_span=None, nll_temperatures=None,
                       adjust=None, item_tag=None, allow_tags=None):
    """Full-catalogue retrieval quality on held-out clicks: per impression of data_iter the targets are its clicked news (the
    ``candidate_ids`` whose label in y_true is 1) and each is ranked against the whole catalogue in recommend()'s own order
    (``model.rank_targets``: the exact position, at any depth).  titles / news_info / exclude_history as in recommend();
    the catalogue is encoded once.  y_true: one 0/1 label list per impression, in data_iter order.

    Returns dict: ``recall@<k>`` and ``ndcg@<k>`` for every k of ks and ``mrr`` (NRMSEngine.retrieval_metrics, unweighted
    means over the users with at least one ranked target), ``median_rank`` (over all ranked targets), ``n_users`` (users
    with a ranked target), ``n_targets`` (ranked targets) and ``n_skipped`` (targets that came back with rank 0: a click
    that is already in the history, a padding or unknown id).  The per-user tensors stay on the device in
    ``last_retrieval_metrics`` (the metrics, plus ``ranks`` [n, T] int32, 0-padded to the widest batch, and ``targets``).
    One host synchronisation, at the end.

    item_bias: ``model.rank_targets``'s per-news prior, so that the metrics describe the order ``recommend`` serves with the
    same prior.  None: the keyword is not passed at all.

    item_time / request_time / window_span (all three or none): recommend()'s time window.  Sample i's targets are ranked against
    the news with request_time[i] - window_span <= item_time[id] <= request_time[i] only (``model.rank_targets(item_time=...,
    window=...)``): the news that were live at the moment of the click, not news that did not exist yet or had long gone.  A
    target outside its window counts as skipped.  For a target inside it the windowed rank is at most the unwindowed one.
    None: the keywords are not passed at all.

    nll_temperatures: None, or up to 8 temperatures T > 0.  The result gains ``nll``: {T: the mean over the ranked targets (the
    ones ``n_targets`` counts) of -log softmax(score / T + item_bias)[target]}, the softmax running over every news the user
    could be recommended (``model.log_prob``; item_bias enters with scale 1), accumulated on the device.  There is no windowed
    partition yet: together with item_time / window_span this raises ValueError.  None: nothing changes, the keyword is not
    passed on and ``nll`` is absent.

    item_tag / allow_tags (both or neither, else ValueError): recommend()'s per-sample tag sets.  Sample i's targets are ranked
    against the news whose tag it allows only (``model.rank_targets_tagged``): Recall@K and MRR "among the news this user may see".
    A held-out target closed by its tag counts as skipped, like one outside its window; the result gains ``n_closed``, the number of
    targets that are skipped for that reason alone (they are in the catalogue, their tag is closed).  Not with a time window or
    nll_temperatures (ValueError naming the keyword).  None: no new keyword reaches the model, the result has no ``n_closed``.

    adjust = (news_ids [n_samples, E], delta [n_samples, E]): recommend()'s per-sample score adjustments.  Sample i's targets are
    ranked in the adjusted order (``model.rank_targets_adjusted``): "Recall@K when seen-but-not-clicked news is demoted".  A target
    whose delta is NaN counts as skipped.  Not with a time window, item_tag / allow_tags or nll_temperatures (ValueError naming the
    keyword).  None: no new keyword reaches the model."""
    net = _inner(model)
    prior = {} if item_bias is None else {"item_bias": item_bias}
    adj = _Adjust("evaluate_retrieval", adjust, (("item_time / request_time / window_span", item_time is not None
                                                  or request_time is not None or window_span is not None),
                                                 ("item_tag / allow_tags", item_tag is not None or allow_tags is not None),
                                                 ("nll_temperatures", nll_temperatures is not None)))
    tags = _TagSets("evaluate_retrieval", item_tag, allow_tags, (("item_time / request_time / window_span", item_time is not None
                                                                  or request_time is not None or window_span is not None),
                                                                 ("nll_temperatures", nll_temperatures is not None)))
    n_closed = None
    nll_t = None
    if nll_temperatures is not None:
        if item_time is not None or request_time is not None or window_span is not None:
            raise ValueError("evaluate_retrieval: nll_temperatures with item_time / request_time / window_span: there is no "
                             "windowed log-partition yet")
        nll_t = [float(t) for t in nll_temperatures]
        if not getattr(type(net), "CATALOGUE_LIKELIHOOD", False):
            raise NotImplementedError("evaluate_retrieval: nll_temperatures needs a model with CATALOGUE_LIKELIHOOD "
                                      "(log_partition / log_prob); %s has none" % type(net).__module__)
    windows = _RequestWindows("evaluate_retrieval", item_time, request_time, window_span)
    ks = tuple(int(k) for k in ks)
    catalogue = net.encode_catalogue(titles, **(news_info or {}))
    dev = catalogue.device
    ranks, targets, done = [], [], 0
    nll_sum = None if nll_t is None else torch.zeros(len(nll_t), dtype=torch.float64, device=dev)
    for datas in data_iter:
        cand = torch.as_tensor(datas["candidate_ids"]).to(dev, dtype=torch.int64)
        B, S = cand.shape
        rows = y_true[done:done + B]
        prior.update(windows.of(done, B, dev))
        done += B
        if len(rows) < B:
            raise ValueError("evaluate_retrieval: %d label rows for %d impressions" % (len(y_true), done))
        width = max(1, max(min(len(y), S) for y in rows))
        lab = np.zeros((B, width), dtype=bool)
        for i, y in enumerate(rows):
            n = min(len(y), S)
            lab[i, :n] = np.asarray(y[:n]) == 1
        # the clicked ids, moved to the front of each row in shown order and padded with -1 to the batch's widest
        T = max(1, int(lab.sum(axis=1).max()))
        lab = torch.from_numpy(lab).to(dev)
        order = torch.argsort((~lab).to(torch.uint8), dim=1, stable=True)[:, :T]
        tg = torch.where(lab.gather(1, order), cand[:, :width].gather(1, order), torch.full_like(order, -1))
        if tags.on:
            tag, allow = tags.of(done - B, B, dev)
            rk, _ = net.rank_targets_tagged(datas, tg, catalogue, tag, allow, exclude_history=exclude_history, **prior)
            # a target of the catalogue whose tag its sample does not allow (on the device, no synchronisation)
            in_cat = (tg >= 1) & (tg < catalogue.shape[0])
            t_tag = tag.to(torch.int64)[tg.clamp(0, catalogue.shape[0] - 1)]
            t_open = (t_tag >= 0) & (t_tag < allow.shape[1]) & allow.gather(1, t_tag.clamp(0, allow.shape[1] - 1))
            closed = (in_cat & ~t_open).sum()
            n_closed = closed if n_closed is None else n_closed + closed
        elif adj.on:
            rk, _ = net.rank_targets_adjusted(datas, tg, catalogue, adj.of(done - B, B, dev), exclude_history=exclude_history, **prior)
        else:
            rk, _ = net.rank_targets(datas, tg, catalogue, exclude_history=exclude_history, **prior)
        ranks.append(rk)
        targets.append(tg)
        if nll_t is not None:
            lp = net.log_prob(datas, tg, catalogue, temperature=nll_t, exclude_history=exclude_history, **prior)
            nll_sum -= torch.where((rk > 0).unsqueeze(-1), lp, torch.zeros_like(lp)).double().sum(dim=(0, 1))
    T = max((r.shape[1] for r in ranks), default=1)
    pad = lambda t, v: torch.nn.functional.pad(t, (0, T - t.shape[1]), value=v)
    ranks = torch.cat([pad(r, 0) for r in ranks]) if ranks else torch.zeros(0, T, dtype=torch.int32, device=dev)
    targets = torch.cat([pad(t, -1) for t in targets]) if targets else torch.zeros(0, T, dtype=torch.int64, device=dev)
    m = net.engine.retrieval_metrics(ranks, ks)
    names = ["recall@%d" % k for k in ks] + ["ndcg@%d" % k for k in ks] + ["mrr"]
    ranked = ranks > 0
    have = ranked.any(dim=1)
    n_users = have.sum()
    flat = torch.where(ranked, ranks, torch.full_like(ranks, torch.iinfo(torch.int32).max)).reshape(-1).sort().values
    n_targets = ranked.sum()
    # median of the ranked ranks (the mean of the middle two when their number is even)
    lo = flat[((n_targets - 1).clamp(min=0) // 2).clamp(max=max(0, flat.numel() - 1))] if flat.numel() else n_targets
    hi = flat[(n_targets // 2).clamp(max=max(0, flat.numel() - 1))] if flat.numel() else n_targets
    vals = [torch.where(have, m[k], torch.zeros_like(m[k])).sum() / n_users.clamp(min=1) for k in names]
    vals += [(lo.double() + hi.double()) / 2, n_users.double(), n_targets.double(), ((targets >= 0) & ~ranked).sum().double()]
    bad = getattr(net, "_bad_browsed", None)
    vals.append(bad.double() if bad is not None else n_users.double() * 0)
    if nll_t is not None:
        vals = list(nll_sum / n_targets.clamp(min=1).double()) + vals
    if tags.on:                                                # (never together with nll_temperatures)
        vals = [n_closed.double() if n_closed is not None else n_users.double() * 0] + vals
    vals = torch.stack(vals).cpu().tolist()                    # the one host synchronisation
    closed = int(vals.pop(0)) if tags.on else None
    nll = None if nll_t is None else dict(zip(nll_t, vals[:len(nll_t)]))
    vals = vals[len(nll_t or ()):]
    net.engine.check_ids()                                     # (its count is on the host by now)
    if vals.pop():
        net.check_recommend_ids()                              # raises: browsed ids outside the catalogue
    res = dict(zip(names, vals[:len(names)]))
    if tags.on:
        res["n_closed"] = closed
    res["median_rank"] = vals[-4]
    res["n_users"], res["n_targets"], res["n_skipped"] = int(vals[-3]), int(vals[-2]), int(vals[-1])
    if not res["n_users"]:
        for k in names + ["median_rank"]:
            res[k] = float("nan")
    if nll is not None:
        res["nll"] = nll if res["n_targets"] else {t: float("nan") for t in nll}
    net.last_retrieval_metrics = dict(m, ranks=ranks, targets=targets)
    if verbose:
        print("retrieval over {} news: ".format(int(catalogue.shape[0]) - 1)
              + "  ".join("{}: {:.4f}".format(k, res[k]) for k in names)
              + "  median rank: {:.1f}  users: {}  targets: {}  skipped: {}".format(res["median_rank"], res["n_users"],
                                                                                   res["n_targets"], res["n_skipped"])
              + ("  closed by tag: {}".format(res["n_closed"]) if tags.on else "")
              + "".join("  nll@T={:g}: {:.4f}".format(t, v) for t, v in (res.get("nll") or {}).items()))
    return res


def _request_parts(who, item_time, request_time, window_span, item_tag, allow_tags, adjust):
    """The per-sample parts of recommend_request() / evaluate_retrieval_request(): the helpers of recommend(), none of which refuses
    another here.  -> (windows, tags, adj)."""
    return (_RequestWindows(who, item_time, request_time, window_span), _TagSets(who, item_tag, allow_tags, ()),
            _Adjust(who, adjust, ()))


def _request_keywords(windows, tags, adj, done, B, dev):
    """The parts' slices for samples [done, done + B) as keywords of ``model.recommend_request`` / ``rank_targets_request``."""
    kw = dict(windows.of(done, B, dev))
    if tags.on:
        kw["item_tag"], kw["allow"] = tags.of(done, B, dev)
    if adj.on:
        kw["adjust"] = adj.of(done, B, dev)
    return kw


def recommend_request(config, model, data_iter, titles, k, out_file=None, exclude_history=True, news_info=None, item_bias=None,
                      item_time=None, request_time=None, window_span=None, item_tag=None, allow_tags=None, adjust=None,
                      tag_caps=None, heldout=None):
    """recommend() through several catalogue filters at once: writes the same ``<impression index> [id1,id2,...]`` lines, per
    impression of data_iter the k news ids ``model.recommend_request`` serves, best first.  titles / news_info / exclude_history /
    item_bias as in recommend().  The parts are recommend()'s keywords, with their rules, and any of them may be given together:
    item_time / request_time / window_span (all three or none), item_tag / allow_tags (both or neither), adjust.  Each is sliced per
    batch, one row per sample of data_iter in its order.  With no part or one part the file is recommend()'s with that keyword,
    byte for byte.  Not with diversity, coarse, explain or sections (they are not keywords here).

    tag_caps (with item_tag; allow_tags optional), heldout (with tag_caps only): recommend()'s cap keywords, with any of the parts
    above: ``model.recommend_request_capped``, the capped walk over the news every part leaves open.  The call leaves
    ``net.last_caps_stats`` as recommend(tag_caps=) does (None without tag_caps).  Returns the file name."""
    net = _inner(model)
    prior = {} if item_bias is None else {"item_bias": item_bias}
    caps = _TagCaps("recommend_request", tag_caps, item_tag, allow_tags, heldout, ())
    # with caps item_tag goes with them, and a tag set needs allow_tags alone
    windows, tags, adj = _request_parts("recommend_request", item_time, request_time, window_span,
                                        None if caps.on and allow_tags is None else item_tag, allow_tags, adjust)
    hit_ks = tuple(kk for kk in (1, 5, 10, 20, 50, 100) if kk < int(k)) + (int(k),)
    catalogue = net.encode_catalogue(titles, **(news_info or {}))
    lines, done = [], 0
    for datas in data_iter:
        B = int(torch.as_tensor(datas["browsed_ids"]).shape[0])
        kw = _request_keywords(windows, tags, adj, done, B, catalogue.device)
        if caps.on:
            tag, cap = caps.of(done, B, catalogue.device)
            kw.pop("item_tag", None)
            ids, _ = net.recommend_request_capped(datas, k, catalogue, tag, cap, exclude_history=exclude_history, **prior, **kw)
            caps.note(done, ids, hit_ks)
            done += B
            lines.extend(ids.cpu().tolist())
            continue
        done += B
        ids, _ = net.recommend_request(datas, k, catalogue, exclude_history=exclude_history, **prior, **kw)
        lines.extend(ids.cpu().tolist())
    net.last_caps_stats = caps.stats(hit_ks) if caps.on else None
    net.engine.check_ids()
    net.check_recommend_ids()
    file_name = out_file or 'recommend_{}_{}.txt'.format(config.model_name, time.strftime('%m-%d_%H.%M', time.localtime()))
    with open(file_name, 'w') as f:
        for i, row in enumerate(lines):
            f.write(str(i + 1) + ' ')
            f.write(str([n for n in row if n >= 0]).replace(' ', '') + '\n')
    return file_name


def evaluate_retrieval_request(config, model, data_iter, titles, y_true, ks=(10, 100), exclude_history=True, news_info=None,
                               verbose=True, item_bias=None, item_time=None, request_time=None, window_span=None, item_tag=None,
                               allow_tags=None, adjust=None):
    """evaluate_retrieval() in the order recommend_request() serves: each held-out click is ranked against the news every part leaves
    open to its sample (``model.rank_targets_request``).  The arguments are evaluate_retrieval()'s, and the parts may be given
    together.  Returns its dict (``recall@<k>``, ``ndcg@<k>``, ``mrr``, ``median_rank``, ``n_users``, ``n_targets``, ``n_skipped``)
    plus ``n_closed``: the held-out clicks of the catalogue that a time window or a tag set closes to their sample; like a click
    with a NaN delta they come back with rank 0 and count as skipped, as in the tagged evaluation.  The per-user tensors stay on
    the device in ``last_retrieval_metrics``.  One host synchronisation, at the end."""
    net = _inner(model)
    prior = {} if item_bias is None else {"item_bias": item_bias}
    windows, tags, adj = _request_parts("evaluate_retrieval_request", item_time, request_time, window_span, item_tag, allow_tags,
                                        adjust)
    ks = tuple(int(k) for k in ks)
    catalogue = net.encode_catalogue(titles, **(news_info or {}))
    dev, N = catalogue.device, int(catalogue.shape[0])
    ranks, targets, done = [], [], 0
    n_closed = torch.zeros((), dtype=torch.int64, device=dev)
    for datas in data_iter:
        cand = torch.as_tensor(datas["candidate_ids"]).to(dev, dtype=torch.int64)
        B, S = cand.shape
        rows = y_true[done:done + B]
        if len(rows) < B:
            raise ValueError("evaluate_retrieval_request: %d label rows for %d impressions" % (len(y_true), done + B))
        kw = _request_keywords(windows, tags, adj, done, B, dev)
        done += B
        width = max(1, max(min(len(y), S) for y in rows))
        lab = np.zeros((B, width), dtype=bool)
        for i, y in enumerate(rows):
            n = min(len(y), S)
            lab[i, :n] = np.asarray(y[:n]) == 1
        # the clicked ids, moved to the front of each row in shown order and padded with -1 to the batch's widest
        T = max(1, int(lab.sum(axis=1).max()))
        lab = torch.from_numpy(lab).to(dev)
        order = torch.argsort((~lab).to(torch.uint8), dim=1, stable=True)[:, :T]
        tg = torch.where(lab.gather(1, order), cand[:, :width].gather(1, order), torch.full_like(order, -1))
        rk, _ = net.rank_targets_request(datas, tg, catalogue, exclude_history=exclude_history, **prior, **kw)
        # a target of the catalogue that its sample's window or tag set closes (on the device, no synchronisation)
        in_cat = (tg >= 1) & (tg < N)
        t_open = torch.ones_like(in_cat)
        if tags.on:
            allow = kw["allow"]
            t_tag = kw["item_tag"].to(torch.int64)[tg.clamp(0, N - 1)]
            t_open &= (t_tag >= 0) & (t_tag < allow.shape[1]) & allow.gather(1, t_tag.clamp(0, allow.shape[1] - 1))
        if windows.on:
            t_time = kw["item_time"].to(torch.int64)[tg.clamp(0, N - 1)]
            w = kw["window"].to(torch.int64)
            t_open &= (t_time >= w[:, :1]) & (t_time < w[:, 1:])
        n_closed += (in_cat & ~t_open).sum()
        ranks.append(rk)
        targets.append(tg)
    T = max((r.shape[1] for r in ranks), default=1)
    pad = lambda t, v: torch.nn.functional.pad(t, (0, T - t.shape[1]), value=v)
    ranks = torch.cat([pad(r, 0) for r in ranks]) if ranks else torch.zeros(0, T, dtype=torch.int32, device=dev)
    targets = torch.cat([pad(t, -1) for t in targets]) if targets else torch.zeros(0, T, dtype=torch.int64, device=dev)
    m = net.engine.retrieval_metrics(ranks, ks)
    names = ["recall@%d" % k for k in ks] + ["ndcg@%d" % k for k in ks] + ["mrr"]
    ranked = ranks > 0
    have = ranked.any(dim=1)
    n_users = have.sum()
    flat = torch.where(ranked, ranks, torch.full_like(ranks, torch.iinfo(torch.int32).max)).reshape(-1).sort().values
    n_targets = ranked.sum()
    # median of the ranked ranks (the mean of the middle two when their number is even)
    lo = flat[((n_targets - 1).clamp(min=0) // 2).clamp(max=max(0, flat.numel() - 1))] if flat.numel() else n_targets
    hi = flat[(n_targets // 2).clamp(max=max(0, flat.numel() - 1))] if flat.numel() else n_targets
    vals = [torch.where(have, m[k], torch.zeros_like(m[k])).sum() / n_users.clamp(min=1) for k in names]
    vals += [(lo.double() + hi.double()) / 2, n_users.double(), n_targets.double(), ((targets >= 0) & ~ranked).sum().double(),
             n_closed.double()]
    bad = getattr(net, "_bad_browsed", None)
    vals.append(bad.double() if bad is not None else n_users.double() * 0)
    vals = torch.stack(vals).cpu().tolist()                    # the one host synchronisation
    net.engine.check_ids()
    if vals.pop():
        net.check_recommend_ids()                              # raises: browsed ids outside the catalogue
    res = dict(zip(names, vals[:len(names)]))
    res["median_rank"] = vals[-5]
    res["n_users"], res["n_targets"], res["n_skipped"], res["n_closed"] = int(vals[-4]), int(vals[-3]), int(vals[-2]), int(vals[-1])
    if not res["n_users"]:
        for k in names + ["median_rank"]:
            res[k] = float("nan")
    net.last_retrieval_metrics = dict(m, ranks=ranks, targets=targets)
    if verbose:
        print("retrieval over {} news: ".format(N - 1)
              + "  ".join("{}: {:.4f}".format(k, res[k]) for k in names)
              + "  median rank: {:.1f}  users: {}  targets: {}  skipped: {}  closed by a part: {}".format(
                  res["median_rank"], res["n_users"], res["n_targets"], res["n_skipped"], res["n_closed"]))
    return res
