"""Top-K for a whole dataset (split out of engine.py): the batches of an epoch resident in HBM against frozen weights, one graph replay a
batch.  What SasrecEngine.enqueue_topk does per call is cut where it stops depending on the user (csrc/full_rank.hip
amid_topk_items_f32 / amid_topk_users_f32), and the history sets come from the plan's static sequences on the device
(csrc/own_sets.hip amid_own_from_seq_i64) instead of a torch.sort + mask gather + cumsum whose shape depends on the data."""
from __future__ import annotations

import ctypes
from typing import Optional

import torch

from ._lib import lib

from .plan import SasrecPlan


class TopkMixin:
    def _topk_buffers(self, pl: SasrecPlan, k: int):
        """The plan's own-set buffers (own [B T] int64, own_off [B + 1], scratch counts [B], rows 0 .. B - 1: int32) and its static
        result buffers for this k (ids [B, k] int64, scores [B, k]); allocated once."""
        B, T = pl.shape.B, pl.shape.T
        fresh = False
        if not hasattr(pl, "tk_own"):
            dev = self.device
            pl.tk_own = torch.zeros(B * T, dtype=torch.int64, device=dev)
            pl.tk_own_off = torch.zeros(B + 1, dtype=torch.int32, device=dev)
            pl.tk_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
            pl.tk_rows = torch.arange(B, dtype=torch.int32, device=dev)
            pl.tk_out = {}
            fresh = True
        if k not in pl.tk_out:
            pl.tk_out[k] = (torch.zeros(B, k, dtype=torch.int64, device=self.device), torch.zeros(B, k, dtype=torch.float32, device=self.device))
            fresh = True
        if fresh:
            torch.cuda.synchronize(self.device)
        return pl.tk_out[k]

    def enqueue_topk_items(self, pl: SasrecPlan, pools, k: int) -> None:
        """The item halves of both pools' candidates into the engine's top-K workspace, for the weights as they are now: one launch
        (amid_topk_items_f32).  enqueue_topk_batch reads them until the workspace, the pools or the weights change."""
        B = pl.shape.B
        p1, p2 = pools
        ws = self._full_rank_workspace(B, p1.numel(), p2.numel(), int(k))
        lib().call("amid_topk_items_f32", B, p1.data_ptr(), p1.numel(), p2.data_ptr(), p2.numel(), self.table.data_ptr(), self.n_rows,
                   self._scorer()["w1"], self.D, self.hid, ws.data_ptr(), pl.err.data_ptr(), self.s)
        self._tk_items = (ws.data_ptr(), B, p1.data_ptr(), p1.numel(), p2.data_ptr(), p2.numel())

    def enqueue_topk_batch(self, pl: SasrecPlan, pools, k: int, exclude_history: bool, ids: torch.Tensor, scores: torch.Tensor,
                           build_images: bool = True) -> None:
        """enqueue_topk for the batch in the plan's static inputs, without its items launch and without a host-built history set: the
        user vectors (enqueue_user_vectors: the launches recommend() uses, so the same bits), with exclude_history the rows' own sets from
        pl.in_seq_d1 / pl.in_seq_d2 / pl.domain (amid_own_from_seq_i64: two launches), amid_topk_users_f32 (three) on the item halves
        enqueue_topk_items left in the workspace for these pools.  ids [B, k] int64, scores [B, k].  Fixed shapes, no host read, no
        allocation once _topk_buffers has run: capturable."""
        L, s, shp = lib(), self.s, pl.shape
        B = shp.B
        p1, p2 = pools
        self._topk_buffers(pl, int(k))
        ws = self._full_rank_workspace(B, p1.numel(), p2.numel(), int(k))
        if getattr(self, "_tk_items", None) != (ws.data_ptr(), B, p1.data_ptr(), p1.numel(), p2.data_ptr(), p2.numel()):
            raise ValueError("enqueue_topk_batch: the workspace holds no item halves for these pools and this batch size (enqueue_topk_items)")
        u, stride = self.enqueue_user_vectors(pl, build_images=build_images)
        if exclude_history:
            L.call("amid_own_from_seq_i64", pl.in_seq_d1.data_ptr(), pl.in_seq_d2.data_ptr(), pl.domain.data_ptr(), B, shp.T,
                   pl.tk_cnt.data_ptr(), pl.tk_own.data_ptr(), pl.tk_own_off.data_ptr(), s)
        L.call("amid_topk_users_f32", u.data_ptr(), stride, pl.domain.data_ptr(), B, p1.data_ptr(), p1.numel(), p2.data_ptr(), p2.numel(),
               pl.tk_own.data_ptr(), pl.tk_own_off.data_ptr(), pl.tk_rows.data_ptr(), self.table.data_ptr(), self.n_rows,
               *self._scorer().values(), self.D, self.hid, int(k), 1 if exclude_history else 0, ws.data_ptr(), pl.err.data_ptr(),
               ids.data_ptr(), scores.data_ptr(), s)

    def capture_topk(self, pl: SasrecPlan, pools, k: int, exclude_history: bool) -> None:
        """enqueue_topk_batch as a hipGraph over the plan's static inputs and result buffers, after enqueue_topk_items for these pools.
        One stream, no parallel branch.  Parameters, the item halves and the weight images are read at replay time (topk_epoch rebuilds the
        latter two before its first replay), so the graph stays valid across train steps; the pools' and the workspace's addresses are baked
        in (topk_epoch captures again when either moved).  Keyed by (k, exclude_history, pool sizes)."""
        L = lib()
        ids, scores = self._topk_buffers(pl, int(k))
        self.enqueue_topk_batch(pl, pools, k, exclude_history, ids, scores)      # warm-up outside capture (LDS attributes, lazy buffers, images)
        self.sync()
        L.call("amid_graph_capture_begin", self.s)
        try:
            self.enqueue_topk_batch(pl, pools, k, exclude_history, ids, scores, build_images=False)
        finally:
            out = ctypes.c_void_p()
            L.call("amid_graph_capture_end", self.s, ctypes.byref(out))
        if not hasattr(pl, "topk_graphs"):
            pl.topk_graphs = {}
        p1, p2 = pools
        key = (int(k), bool(exclude_history), p1.numel(), p2.numel())
        old = pl.topk_graphs.get(key)
        if old is not None:
            L.call("amid_graph_destroy", old[0])
        # (the pools are kept alive with the graph that reads them)
        pl.topk_graphs[key] = (out.value, self._tk_items, (p1, p2))

    def topk_epoch(self, pl: SasrecPlan, packed: torch.Tensor, pools, k: int, exclude_history: bool, use_graph: bool = True):
        """Every batch of `packed` ([n, in_words] int64: pack_epoch's images with zero i_node and one zero negative per row, resident in
        HBM) through the top-K launches: the lazy table flushed, the weight images and the pools' item halves built ONCE, then per batch
        one device copy of the image into the plan's static inputs, one graph replay (use_graph=False: the same launches, eagerly) and
        two device copies of the results out.  Returns (ids [n, B, k] int64, scores [n, B, k] float32) on the device; nothing is read back.
        Where eval_fused_ok(pl) is false the user vectors are enqueue_prepare + enqueue_forward; that sequence is plain launches on the
        engine's stream for an evaluation-mode batch on one GPU and is captured like the fused one."""
        if packed.dtype != torch.int64 or packed.dim() != 2 or packed.shape[1] != pl.in_words:
            raise ValueError(f"topk_epoch takes [n, {pl.in_words}] int64 batch images (pack_epoch)")
        if self.table_m is not None:
            self.flush_table()                   # rows with pending zero-gradient Adam steps must be current
        L, k = lib(), int(k)
        n, B = packed.shape[0], pl.shape.B
        p1, p2 = pools
        ids = torch.empty(n, B, k, dtype=torch.int64, device=self.device)
        scores = torch.empty(n, B, k, dtype=torch.float32, device=self.device)
        b_ids, b_scores = self._topk_buffers(pl, k)
        fused = self.eval_fused_ok(pl)
        with torch.cuda.stream(self.stream):
            if fused:
                self._enqueue_eval_images(pl)        # this epoch's weight images, once (the batches' launches only read them)
            self.enqueue_topk_items(pl, pools, k)
        key = (k, bool(exclude_history), p1.numel(), p2.numel())
        if use_graph:
            ent = getattr(pl, "topk_graphs", {}).get(key)
            if ent is None or ent[1] != self._tk_items:
                with torch.cuda.stream(self.stream):
                    pl.in_pack.copy_(packed[0], non_blocking=True)
                self.capture_topk(pl, pools, k, exclude_history)
        with torch.cuda.stream(self.stream):
            for i in range(n):
                pl.in_pack.copy_(packed[i], non_blocking=True)
                if use_graph:
                    L.call("amid_graph_launch", pl.topk_graphs[key][0], self.s)
                else:
                    self.enqueue_topk_batch(pl, pools, k, exclude_history, b_ids, b_scores, build_images=False)
                ids[i].copy_(b_ids, non_blocking=True)
                scores[i].copy_(b_scores, non_blocking=True)
        return ids, scores

    # ------------------------------------------------------------------ audience top-K: the users of an item (csrc/audience.hip)
    AUDIENCE_CHUNK = 1024         # query items per amid_audience_topk_f32 call at most (the workspace is sized for it)

    def _audience_workspace(self, Q: int, n1: int, n2: int, k: int) -> torch.Tensor:
        nbytes = int(lib().value("amid_audience_workspace_bytes", Q, n1, n2, self.hid, k))
        if nbytes < 0:
            raise ValueError(f"audience top-K: bad sizes Q {Q}, rows {n1} / {n2}, k {k}")
        ws = getattr(self, "_au_ws", None)
        if ws is None or ws.numel() < nbytes:
            if ws is not None:
                ws.record_stream(self.stream)          # (launches still queued on the engine's stream may read the old one)
            with torch.cuda.stream(self.stream):
                ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._au_ws = ws
        return ws

    def enqueue_audience_halves(self, vectors: torch.Tensor, slots) -> None:
        """The user halves W1[:, :D] v + b1 of the listed rows of vectors [N, D] (contiguous float32 on the device) into the audience
        workspace, for the weights as they are now: one launch (amid_audience_halves_f32).  slots = (domain 0's rows, domain 1's rows):
        ascending int32 device tensors, not both empty.  The workspace is grown here to what any later enqueue_audience_topk on these
        lists needs (AUDIENCE_CHUNK queries, k = 256), so it does not move between the two.  Nothing is synchronised."""
        s1, s2 = slots
        ws = self._audience_workspace(self.AUDIENCE_CHUNK, s1.numel(), s2.numel(), 256)
        flags = self.flags_holder()
        sc = self._scorer()
        lib().call("amid_audience_halves_f32", vectors.data_ptr(), vectors.shape[0], s1.data_ptr() if s1.numel() else None, s1.numel(),
                   s2.data_ptr() if s2.numel() else None, s2.numel(), sc["w1"], sc["b1"], self.D, self.hid, ws.data_ptr(), flags.err.data_ptr(),
                   self.s)
        self._au_halves = (ws.data_ptr(), s1.data_ptr(), s1.numel(), s2.data_ptr(), s2.numel())

    def enqueue_audience_topk(self, items: torch.Tensor, item_domain: torch.Tensor, slots, holders, k: int, rows: torch.Tensor,
                              scores: torch.Tensor, err: torch.Tensor) -> None:
        """amid_audience_topk_f32 on the engine's stream: for each query item (items, item_domain [Q] int64, Q <= AUDIENCE_CHUNK) the k
        best rows of its domain's list among those enqueue_audience_halves prepared for these `slots`, minus holders -- None, or
        (indices int32 ascending within a query, offsets [Q + 1] int64 into indices); rows [Q, k] int64, scores [Q, k], err [1] int32
        flags.  Nothing is synchronised."""
        s1, s2 = slots
        Q = items.shape[0]
        if Q > self.AUDIENCE_CHUNK:
            raise ValueError(f"enqueue_audience_topk: at most {self.AUDIENCE_CHUNK} queries a call, got {Q}")
        ws = self._audience_workspace(Q, s1.numel(), s2.numel(), int(k))
        if getattr(self, "_au_halves", None) != (ws.data_ptr(), s1.data_ptr(), s1.numel(), s2.data_ptr(), s2.numel()):
            raise ValueError("enqueue_audience_topk: the workspace holds no user halves for these slot lists (enqueue_audience_halves)")
        sc = self._scorer()
        hold, hold_off = (None, None) if holders is None else (holders[0].data_ptr() if holders[0].numel() else None, holders[1].data_ptr())
        if holders is not None and hold is None:
            hold_off = None                               # (every list is empty)
        lib().call("amid_audience_topk_f32", items.data_ptr(), item_domain.data_ptr(), Q, self.table.data_ptr(), self.n_rows, sc["w1"],
                   sc["w2"], sc["b2"], s1.data_ptr() if s1.numel() else None, s1.numel(), s2.data_ptr() if s2.numel() else None, s2.numel(),
                   hold, hold_off, self.D, self.hid, int(k), ws.data_ptr(), err.data_ptr(), rows.data_ptr(), scores.data_ptr(), self.s)

    # ------------------------------------------------------------------ ranking each row's own candidate list (csrc/rank_lists.hip)
    def _rank_lists_workspace(self, B: int, n_cand: int, k: int) -> torch.Tensor:
        nbytes = int(lib().value("amid_rank_lists_workspace_bytes", B, n_cand, self.hid, k))
        if nbytes < 0:
            raise ValueError(f"rank lists: bad sizes B {B}, candidates {n_cand}, k {k}")
        ws = getattr(self, "_rl_ws", None)
        if ws is None or ws.numel() < nbytes:
            if ws is not None:
                ws.record_stream(self.stream)          # (launches still queued on the engine's stream may read the old one)
            with torch.cuda.stream(self.stream):
                ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._rl_ws = ws
        return ws

    def enqueue_own_sets(self, seq_d1: torch.Tensor, seq_d2: torch.Tensor, domain: torch.Tensor):
        """own(b) = the sorted unique ids of row b's own-domain sequence (seq_d1 / seq_d2 [B, T] int64, domain [B]) as amid_topk_f32's
        history triple (own, own_off, rows), formed on the device (amid_own_from_seq_i64).  Nothing is synchronised."""
        B, T = seq_d1.shape
        with torch.cuda.stream(self.stream):
            own = torch.empty(B * T, dtype=torch.int64, device=self.device)
            own_off = torch.empty(B + 1, dtype=torch.int32, device=self.device)
            cnt = torch.empty(B, dtype=torch.int32, device=self.device)
            rows = torch.arange(B, dtype=torch.int32, device=self.device)
        lib().call("amid_own_from_seq_i64", seq_d1.data_ptr(), seq_d2.data_ptr(), domain.data_ptr(), B, T, cnt.data_ptr(), own.data_ptr(),
                   own_off.data_ptr(), self.s)
        return own, own_off, rows

    def enqueue_rank_lists(self, u: torch.Tensor, u_dom_stride: int, domain: torch.Tensor, cand: torch.Tensor, cand_off: torch.Tensor,
                           n_cand: int, own: Optional[torch.Tensor], own_off: Optional[torch.Tensor], rows: Optional[torch.Tensor], k,
                           list_scores: Optional[torch.Tensor], ids: Optional[torch.Tensor], scores: Optional[torch.Tensor],
                           positions: Optional[torch.Tensor], err: torch.Tensor) -> None:
        """amid_rank_lists_f32 on the engine's stream: row b's vector (u + domain[b] * u_dom_stride + b * D floats: what
        enqueue_user_vectors returns fits, or [B, D] vectors with stride 0) against its own list cand[cand_off[b] : cand_off[b + 1]]
        (cand int64 [n_cand], cand_off int64 [B + 1] on the device, n_cand the host's copy of cand_off[B]).  list_scores [n_cand] or None;
        ids / scores / positions [B, k] or all None (k is then ignored); own / own_off / rows: amid_topk_f32's history triple or None;
        err [1] int32 flags.  Nothing is synchronised."""
        B = domain.shape[0]
        k = int(k) if ids is not None else 0
        ws = self._rank_lists_workspace(B, int(n_cand), k)
        ptr = lambda t: None if t is None or t.numel() == 0 else t.data_ptr()       # noqa: E731
        lib().call("amid_rank_lists_f32", u.data_ptr(), int(u_dom_stride), domain.data_ptr(), B, ptr(cand), cand_off.data_ptr(), int(n_cand),
                   ptr(own), None if own is None else own_off.data_ptr(), None if own is None else rows.data_ptr(), self.table.data_ptr(),
                   self.n_rows, *self._scorer().values(), self.D, self.hid, k, ws.data_ptr(), err.data_ptr(), ptr(list_scores),
                   None if ids is None else ids.data_ptr(), None if scores is None else scores.data_ptr(),
                   None if positions is None else positions.data_ptr(), self.s)

    # ------------------------------------------------------------------ diversified top-K: greedy MMR over each row's list (csrc/diversify.hip)
    def _mmr_workspace(self, B: int, n_cand: int, k: int, shortlist: int) -> torch.Tensor:
        nbytes = int(lib().value("amid_mmr_workspace_bytes", B, n_cand, self.D, k, shortlist))
        if nbytes < 0:
            raise ValueError(f"diversify: bad sizes B {B}, candidates {n_cand}, k {k}, shortlist {shortlist}, D {self.D}")
        ws = getattr(self, "_mmr_ws", None)
        if ws is None or ws.numel() < nbytes:
            if ws is not None:
                ws.record_stream(self.stream)          # (launches still queued on the engine's stream may read the old one)
            with torch.cuda.stream(self.stream):
                ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._mmr_ws = ws
        return ws

    def enqueue_mmr_lists(self, cand: torch.Tensor, cand_off: torch.Tensor, rel: torch.Tensor, n_cand: int, metric: str, lam: float, k: int,
                          shortlist: int, ids: torch.Tensor, scores: torch.Tensor, values: torch.Tensor, max_sims: torch.Tensor,
                          positions: torch.Tensor, err: torch.Tensor) -> None:
        """amid_mmr_lists_f32 on the engine's stream over the item table: row b's list cand[cand_off[b] : cand_off[b + 1]] (cand int64
        [n_cand], cand_off int64 [B + 1] on the device, n_cand the host's copy of cand_off[B]) with the relevance rel [n_cand] float32;
        ids / scores / values / max_sims / positions [B, k]; err [1] int32 flags.  Nothing is synchronised."""
        B = cand_off.shape[0] - 1
        ws = self._mmr_workspace(B, int(n_cand), int(k), int(shortlist))
        ptr = lambda t: None if t.numel() == 0 else t.data_ptr()                     # noqa: E731
        lib().call("amid_mmr_lists_f32", ptr(cand), cand_off.data_ptr(), ptr(rel), int(n_cand), B, self.table.data_ptr(), self.n_rows, self.D,
                   self.NEIGHBOR_METRICS[metric], float(lam), int(k), int(shortlist), ws.data_ptr(), err.data_ptr(), ids.data_ptr(),
                   scores.data_ptr(), values.data_ptr(), max_sims.data_ptr(), positions.data_ptr(), self.s)
