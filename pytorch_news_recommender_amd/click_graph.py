"""The click graph of a whole data set, resident in HBM, and the neighbour sampler over it (``nrms_graph_sample_neighbors`` /
``nrms_graph_resolve_rows``, csrc/graphsample.hip) -- the global counterpart of ``graph_sampler.induced_neighbor_rows`` for the
user-news graph encoder (model/graph_hip.py).  PARITY UNPINNED: the reference has no graph model.

``ClickGraph`` holds the bipartite user-news graph as two CSRs on one device:

  ``user_ptr`` [U + 1] int64, ``user_news`` [E] int32 -- the distinct news a user clicked, ascending id;
  ``news_ptr`` [n_news + 1] int64, ``news_users`` [E] int32 -- the distinct users who clicked a news, ascending id.

News id 0 (the padding slot of a history) and ids outside [0, n_news) are never edges; ``n_padding`` and ``n_out_of_range`` say how
many of each the histories held.  The graph is built once at set-up (torch sort / unique on the device: plumbing); sampling is HIP,
a pure function of (graph, news id, draw, seed) -- see include/nrms_hip.h for the five steps of a draw.  No CPU path for sampling.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

I31 = 2 ** 31 - 1


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check_csr(name, ptr, idx):
    for label, t, dt in ((name + "_ptr", ptr, torch.int64), (name + " index list", idx, torch.int32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != 1:
            raise _lib.NrmsError("ClickGraph: %s must be a 1-d %s tensor, got %s" % (
                label, dt, "%s%s" % (t.dtype, tuple(t.shape)) if isinstance(t, torch.Tensor) else type(t).__name__))
    if ptr.numel() < 1:
        raise _lib.NrmsError("ClickGraph: %s_ptr must hold at least one entry" % name)


class ClickGraph:
    def __init__(self, user_ptr, user_news, news_ptr, news_users, n_padding=0, n_out_of_range=0):
        _check_csr("user", user_ptr, user_news)
        _check_csr("news", news_ptr, news_users)
        n_users, n_news = user_ptr.numel() - 1, news_ptr.numel() - 1
        if not 1 <= n_news <= I31:
            raise _lib.NrmsError("ClickGraph: n_news = %d must be in [1, 2^31 - 1]" % n_news)
        if n_users > I31:
            raise _lib.NrmsError("ClickGraph: %d users: a news may have a degree above 2^31 - 1" % n_users)
        if user_news.numel() != news_users.numel():
            raise _lib.NrmsError("ClickGraph: the two CSRs hold %d and %d edges" % (user_news.numel(), news_users.numel()))
        if len({t.device for t in (user_ptr, user_news, news_ptr, news_users)}) != 1:
            raise _lib.NrmsError("ClickGraph: the four arrays must live on one device")
        self.user_ptr, self.user_news = user_ptr.contiguous(), user_news.contiguous()
        self.news_ptr, self.news_users = news_ptr.contiguous(), news_users.contiguous()
        self.n_users, self.n_news, self.n_edges = n_users, n_news, user_news.numel()
        self.n_padding, self.n_out_of_range = int(n_padding), int(n_out_of_range)
        self.device = user_ptr.device
        self._ws = None
        # device counters of sample_neighbors / resolve_rows calls that pass none of their own
        self.bad_slot_ids = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.dropped_extra = torch.zeros(1, dtype=torch.int32, device=self.device)

    @classmethod
    def from_histories(cls, hist_ids, n_news, device=None):
        """hist_ids [U, H] integer news ids (row u = the clicks of user u, 0 = padding slot) -> the graph on ``device``
        (default: where hist_ids lives).  Duplicate clicks of a user are one edge."""
        if not isinstance(hist_ids, torch.Tensor):
            try:
                hist_ids = torch.as_tensor(hist_ids)
            except Exception as e:
                raise _lib.NrmsError("ClickGraph.from_histories: hist_ids is not a tensor (%s)" % e)
        if hist_ids.dtype not in (torch.int32, torch.int64) or hist_ids.dim() != 2:
            raise _lib.NrmsError("ClickGraph.from_histories: hist_ids must be [U, H] int32 or int64, got %s%s"
                                 % (hist_ids.dtype, tuple(hist_ids.shape)))
        if isinstance(n_news, bool) or not isinstance(n_news, int) or not 1 <= n_news <= I31:
            raise _lib.NrmsError("ClickGraph.from_histories: n_news = %r must be an int in [1, 2^31 - 1]" % (n_news,))
        U, H = hist_ids.shape
        if U > I31 or H > I31:
            # a user's degree is at most H, a news's at most U
            raise _lib.NrmsError("ClickGraph.from_histories: %d users x %d slots allow a degree above 2^31 - 1" % (U, H))
        ids = hist_ids.to(device if device is not None else hist_ids.device, dtype=torch.int64)
        dev = ids.device
        outside = (ids < 0) | (ids >= n_news)
        live = ~outside & (ids != 0)
        user = torch.arange(U, device=dev, dtype=torch.int64)[:, None].expand(U, H)[live]
        news = ids[live]
        by_user = torch.unique(user * n_news + news)                       # sorted: user-major, a user's news ascending
        e_user, e_news = by_user // n_news, by_user % n_news
        by_news = torch.sort(e_news * max(U, 1) + e_user).values           # news-major, a news's users ascending
        zero = torch.zeros(1, dtype=torch.int64, device=dev)
        user_ptr = torch.cat([zero, torch.cumsum(torch.bincount(e_user, minlength=U), 0)])
        news_ptr = torch.cat([zero, torch.cumsum(torch.bincount(e_news, minlength=n_news), 0)])
        return cls(user_ptr, e_news.to(torch.int32), news_ptr, (by_news % max(U, 1)).to(torch.int32),
                   n_padding=int((ids == 0).sum()), n_out_of_range=int(outside.sum()))

    def nbytes(self):
        """Footprint of the four arrays."""
        return sum(t.numel() * t.element_size() for t in (self.user_ptr, self.user_news, self.news_ptr, self.news_users))

    def _desc(self):
        return _lib.ClickGraphDesc(n_users=self.n_users, n_news=self.n_news, n_edges=self.n_edges, user_ptr=self.user_ptr.data_ptr(),
                                   user_news=self.user_news.data_ptr(), news_ptr=self.news_ptr.data_ptr(), news_users=self.news_users.data_ptr())

    def _need_gpu(self, what, *tensors):
        if self.device.type != "cuda":
            raise _lib.NrmsError("ClickGraph.%s: the graph is on %s; sampling runs on a GPU (there is no CPU path)" % (what, self.device))
        for t in tensors:
            if t.device != self.device:
                raise _lib.NrmsError("ClickGraph.%s: an argument is on %s, the graph on %s" % (what, t.device, self.device))

    def sample_neighbors(self, slot_ids, K, seed, n_bad=None):
        """slot_ids [N] int64 news ids on the graph's device -> neighbor_ids [N, K] int32 (-1 = no neighbour).  n_bad: device
        int32 [1] that receives the number of slot ids outside [0, n_news) (default: ``self.bad_slot_ids``)."""
        if not isinstance(slot_ids, torch.Tensor) or slot_ids.dtype != torch.int64 or slot_ids.dim() != 1:
            raise _lib.NrmsError("ClickGraph.sample_neighbors: slot_ids must be a 1-d int64 tensor")
        if isinstance(K, bool) or not isinstance(K, int) or not 1 <= K <= 64:
            raise _lib.NrmsError("ClickGraph.sample_neighbors: K = %r must be an int in [1, 64]" % (K,))
        if slot_ids.numel() * K > I31:
            raise _lib.NrmsError("ClickGraph.sample_neighbors: %d slots x %d draws exceed 2^31 - 1" % (slot_ids.numel(), K))
        self._need_gpu("sample_neighbors", slot_ids)
        lib = _lib.load()
        slot_ids = slot_ids.contiguous()
        N = slot_ids.numel()
        if n_bad is None:
            n_bad = self.bad_slot_ids
        out = torch.empty(N, K, dtype=torch.int32, device=self.device)
        desc = self._desc()
        rc = lib.nrms_graph_sample_neighbors(C.byref(desc), C.c_int64(N), K, _lib.ptr(slot_ids), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
                                             _lib.ptr(out), _lib.ptr(n_bad), None, C.c_size_t(0), _stream())
        _lib.check(rc, "nrms_graph_sample_neighbors")
        return out

    def resolve_rows(self, slot_ids, neighbor_ids, cap, n_dropped=None):
        """Neighbour news ids -> (neighbor_rows [N, K] int64, extra_ids [cap] int32, n_extra int32 [1]): rows < N are slots of
        the batch, row N + e is out-of-batch news extra_ids[e] (include/nrms_hip.h).  n_dropped: device int32 [1] that
        accumulates the distinct out-of-batch ids beyond ``cap`` (default: ``self.dropped_extra``)."""
        if not isinstance(neighbor_ids, torch.Tensor) or neighbor_ids.dtype != torch.int32 or neighbor_ids.dim() != 2:
            raise _lib.NrmsError("ClickGraph.resolve_rows: neighbor_ids must be [N, K] int32")
        if not isinstance(slot_ids, torch.Tensor) or slot_ids.dtype != torch.int64 or slot_ids.shape != neighbor_ids.shape[:1]:
            raise _lib.NrmsError("ClickGraph.resolve_rows: slot_ids must be int64 [N = %d]" % neighbor_ids.shape[0])
        N, K = neighbor_ids.shape
        if isinstance(cap, bool) or not isinstance(cap, int) or cap < 0 or N + cap > I31:
            raise _lib.NrmsError("ClickGraph.resolve_rows: cap = %r must be an int in [0, 2^31 - 1 - N]" % (cap,))
        if not 1 <= K <= 64:
            raise _lib.NrmsError("ClickGraph.resolve_rows: K = %d must be in [1, 64]" % K)
        self._need_gpu("resolve_rows", slot_ids, neighbor_ids)
        lib = _lib.load()
        nbytes = int(lib.nrms_graph_resolve_workspace_bytes(C.c_int64(self.n_news)))
        if self._ws is None or self._ws.numel() * 4 < nbytes:
            self._ws = torch.empty((nbytes + 3) // 4, dtype=torch.int32, device=self.device)
        if n_dropped is None:
            n_dropped = self.dropped_extra
        rows = torch.empty(N, K, dtype=torch.int64, device=self.device)
        extra = torch.empty(cap, dtype=torch.int32, device=self.device)
        n_extra = torch.empty(1, dtype=torch.int32, device=self.device)
        rc = lib.nrms_graph_resolve_rows(C.c_int64(N), K, C.c_int64(self.n_news), _lib.ptr(slot_ids.contiguous()), _lib.ptr(neighbor_ids.contiguous()),
                                         cap, _lib.ptr(rows), _lib.ptr(extra) if cap else None, _lib.ptr(n_extra), _lib.ptr(n_dropped),
                                         _lib.ptr(self._ws), C.c_size_t(self._ws.numel() * 4), _stream())
        _lib.check(rc, "nrms_graph_resolve_rows")
        return rows, extra, n_extra
