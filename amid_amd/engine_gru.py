"""Host-side driver of the GRU4Rec variant of the hot path (reference: GRU4Rec model_seq.py:56-113; training loop train_sr.py:190-217).
Same engine as SASRec and BERT4Rec (table, lazy Adam, index sort, segment reduce, scorer head, hipGraph, input pools, fused evaluation,
full-catalog ranking); only the encoder launches (csrc/gru.hip), the saved activations and the dense parameter list differ.

Reference facts kept: one nn.GRU(D, D, 1, batch_first=True, dropout=0.5) per domain -- with one layer that dropout is a no-op, so train and
eval give the same bits and no random number is drawn; h0 = 0; the encoder input is the plain gathered rows (no positional table, no
input dropout, no "== 0" mask: the pad id's row is an ordinary trained row and every one of the T positions is stepped through); the user
vector is the plain mean over all T outputs (model_seq.py:102-104).  D = 128 only (the reference's default; the kernels' tile).

The three switches of the reference's constructor (model_seq.py:58-78), any combination, every batch of exactly bs rows with isInC / isItC:
  inc_bs (isInC, :89-91)  InnerComp on the plain gathered rows in FRONT of the GRUs -- no positional rows, no dropout, no "== 0" mask: the
                          compute-once token group BERT4Rec's isInC uses (amid_bert_comp_*_f32 with cross = 0).  Each GRU then steps through
                          2 T tokens [e[g, b, :] | Z[g]] and the mean runs over all 2 T outputs; the gather layout (T tokens a row, pl.xg) and
                          the encoder layout (2 T, pl.x[0]) are separate buffers, as in SASRec's isInC plan.
  itc_bs (isItC, :97-101) InterComp on the GRU outputs of every step.  The group token is the same for every batch row and only the mean over
                          time follows, so the module collapses onto the per-row means exactly as for SASRec (csrc/intercomp.hip) with f = h
                          and no LayerNorm: amid_itc_pairmax_raw_f32 (s and the plain means), then the mix kernels.  Both domains of every
                          sample are encoded and both receive gradient: no live-sequence list anywhere in such a step.
  dr (isDR, :106-110)     predict_ips / predict_gfunc on the same (u, items); the objectives and the two Adam states as for SASRec."""
from __future__ import annotations

import ctypes
from typing import List, Tuple

import torch

from ._lib import lib, ptr_array
from .engine import SasrecEngine, SasrecPlan

GRU_HIDDEN = 128
N_ENT = 6       # weight-gradient tiles of 128 x 128 per domain: the r, z, n row blocks of W_ih, then of W_hh


def gru4rec_dense_names(D: int, hid: int, itc_bs: int = 0, dr: bool = False, inc_bs: int = 0) -> List[Tuple[str, Tuple[int, ...]]]:
    """Non-table parameters in the reference's state_dict order (the constructor's, model_seq.py:65-78: inc_d*, itc_d*, gru*, the heads)."""
    out: List[Tuple[str, Tuple[int, ...]]] = []
    for comp, bs in (("inc", inc_bs), ("itc", itc_bs)):
        for d in (1, 2) if bs else ():
            out.append((f"{comp}_d{d}.trans_nn.weight", (D, D)))
            out.append((f"{comp}_d{d}.trans_nn.bias", (D,)))
            out.append((f"{comp}_d{d}.trans_bs.weight", (1, bs)))
            out.append((f"{comp}_d{d}.trans_bs.bias", (1,)))
    for d in (1, 2):
        out.append((f"gru{d}.weight_ih_l0", (3 * D, D)))
        out.append((f"gru{d}.weight_hh_l0", (3 * D, D)))
        out.append((f"gru{d}.bias_ih_l0", (3 * D,)))
        out.append((f"gru{d}.bias_hh_l0", (3 * D,)))
    for head in ("predictModule",) + (("predict_ips", "predict_gfunc") if dr else ()):
        out.append((f"{head}.fc.0.weight", (hid, 2 * D)))
        out.append((f"{head}.fc.0.bias", (hid,)))
        out.append((f"{head}.fc.2.weight", (1, hid)))
        out.append((f"{head}.fc.2.bias", (1,)))
    return out


class GruPlan(SasrecPlan):
    # the backward walks the live list itself (amid_gru_rec_bwd_f32 / amid_gru_dx_f32) and tiles live and all sequences alike: one set of
    # partial slots, one reduce table
    LIVE_ROWS_BWD = False

    def _alloc_model_fwd(self, eng, f) -> None:
        M, D = self.shape.M, eng.D
        for flag, bs in (("isInC", eng.inc_bs), ("isItC", eng.itc_bs)):      # (no data-parallel shards of a comp batch: GRU4Rec runs on one GPU)
            if bs and self.shape.B != bs:
                raise ValueError(f"GRU4Rec {flag}: the batch must hold exactly bs = {bs} rows (trans_bs is Linear(bs, 1) over the batch), "
                                 f"got {self.shape.B}")
        if not lib().value("amid_gru_supported", self.shape.B, self.shape.Tenc, D):
            raise ValueError(f"GRU4Rec: batch {self.shape.B} x {self.shape.Tenc} tokens is beyond the recurrence kernels (amid_gru_supported)")
        self.gi = f(2 * M, 3 * D)                      # X W_ih^T + b_ih

    def _alloc_model_bwd(self, eng, f) -> None:
        M, D = self.shape.M, eng.D
        self.gates, self.ghn, self.hprev = f(2 * M, 3 * D), f(2 * M, D), f(2 * M, D)
        self.dgi, self.dgh = f(2 * M, 3 * D), f(2 * M, 3 * D)
        # 2 domains x 6 tiles x splits workgroups of the fp32 matrix instructions: 10 splits = 120 at the headline batch
        self.splits = max(1, min(int(self.WGRAD_SPLITS or 10), M // 128))
        self.w_part = f(2, N_ENT, self.splits, D * D)
        self.b_part = f(2, N_ENT, self.splits, D)

    def _model_reduce_entries(self, eng, add) -> None:
        D, S = eng.D, self.splits
        fp, G = eng.dense, eng.dense.grad
        for g in (0, 1):
            for j, kind in enumerate(("ih", "hh")):
                for c in range(3):      # rows c * 128 ... of a [384, 128] weight are one contiguous 128 x 128 tile
                    e = 3 * j + c
                    add(self.w_part, ((g * N_ENT + e) * S) * D * D, fp.ptr(f"gru{g + 1}.weight_{kind}_l0", G, c * D * D), D * D, S, D * D)
                    add(self.b_part, ((g * N_ENT + e) * S) * D, fp.ptr(f"gru{g + 1}.bias_{kind}_l0", G, c * D), D, S, D)


class Gru4recEngine(SasrecEngine):
    HEADS = 1                    # (no attention: the base plan's per-head statistics shrink to one column)
    PLAN_CLS = GruPlan
    EMB_DIMS = (GRU_HIDDEN,)
    STRIP_KERNELS = True         # (pl.strip: the step's live-sequence list exists; the encoder's own kernels take it)
    SORT_RIDERS = False          # (the riders' host launches are the SASRec strip backward's)
    FUSED_TAIL = False           # (the one-launch step head and the folded tail are the SASRec step's)
    EVAL_FUSED = True            # test() batches as one graph replay (engine.enqueue_eval on this model's encoder: _enqueue_eval_encoders)

    def __init__(self, *args, **kw):
        if kw.get("compute", "f32") != "f32":
            raise ValueError("GRU4Rec: compute must be 'f32' (the recurrence runs on the fp32 matrix instructions only)")
        if kw.get("loss", "bce") != "bce" and kw.get("itc_bs", 0):
            raise ValueError(f"loss = {kw['loss']!r} is refused with GRU4Rec isItC: the listwise step is not built for it")
        super().__init__(*args, **kw)

    def _dense_names(self):
        return gru4rec_dense_names(self.D, self.hid, self.itc_bs, self.dr, self.inc_bs)

    def _alloc_model_buffers(self) -> None:
        pass                     # (the kernels read W_ih / W_hh in place, as A W^T forward and as A W backward: no transposed copies)

    def _fwd_on_pieces(self, pl, B: int, T: int) -> bool:
        return False             # (SASRec's one-launch forward and its weight images)

    def live_forward_ok(self, pl) -> bool:
        """Whether this engine's train step on `pl` encodes the live sequences only (engine._enqueue_fwd_bwd)."""
        return bool(getattr(pl, "strip", False) and not self.itc_bs and not self.dr and not self.inc_bs and self.FUSED_HEAD and self.LIVE_FORWARD
                    and self.loss == "bce")

    # ---- data parallel: not built (the exchange would work unchanged; nothing here has been run at a world above one)
    def train_step_dp(self, pl, exchange, *args, **kw):
        if exchange is not None and exchange.world > 1:
            raise NotImplementedError("GRU4Rec: data-parallel training (world > 1) is not built")
        return super().train_step_dp(pl, exchange, *args, **kw)

    def capture_local_grads(self, pl, *args, **kw):
        raise NotImplementedError("GRU4Rec: data-parallel training (world > 1) is not built")

    # GRU4Rec has no last LayerNorm: the user vectors are the plain means over time (model_seq.py:102-104)
    # isItC: InterComp on the raw GRU outputs -- the pair-max kernel has every row of (b) in LDS and emits the plain means too
    # (mix=False: only that launch -- pl.itc_s and the unmixed pl.u_raw; the evaluation head mixes in its prologue)
    def _enqueue_user_vectors(self, pl, mix: bool = True) -> None:
        L, s, shp, D = lib(), self.s, pl.shape, self.D
        B, T = shp.B, shp.Tenc
        if not self.itc_bs:
            L.call("amid_lnmean_fwd_f32", pl.x[2].data_ptr(), None, None, None, None, B, T, D, 0.0, pl.u.data_ptr(), s)
            return
        L.call("amid_itc_pairmax_raw_f32", pl.x[2].data_ptr(), B, T, D, pl.itc_s.data_ptr(), pl.u_raw.data_ptr(), s)
        if mix:
            L.call("amid_itc_mix_fwd_f32", pl.u_raw.data_ptr(), pl.itc_s.data_ptr(), self._pp("itc_d{d}.trans_nn.weight"),
                   self._pp("itc_d{d}.trans_nn.bias"), self._pp("itc_d{d}.trans_bs.weight"), self._pp("itc_d{d}.trans_bs.bias"),
                   self.itc_threshold, B, D, pl.itc_gate.data_ptr(), pl.itc_z.data_ptr(), pl.itc_sw.data_ptr(), pl.u.data_ptr(), s)

    def _enqueue_user_vectors_bwd(self, pl) -> None:
        L, s, shp, D = lib(), self.s, pl.shape, self.D
        B, T = shp.B, shp.Tenc
        du, G = pl.du, self.dense.grad
        if self.itc_bs:      # pl.du -> the InterComp parameters' gradients (written whole) and the gradient of the plain means
            L.call("amid_itc_mix_bwd_f32", pl.du.data_ptr(), pl.u_raw.data_ptr(), pl.itc_gate.data_ptr(), pl.itc_z.data_ptr(),
                   pl.itc_sw.data_ptr(), self._pp("itc_d{d}.trans_nn.weight"), self._pp("itc_d{d}.trans_nn.bias"),
                   self._pp("itc_d{d}.trans_bs.weight"), B, D, pl.du_raw.data_ptr(), self._pp("itc_d{d}.trans_nn.weight", G),
                   self._pp("itc_d{d}.trans_nn.bias", G), self._pp("itc_d{d}.trans_bs.weight", G), self._pp("itc_d{d}.trans_bs.bias", G), s)
            du = pl.du_raw
        L.call("amid_lnmean_bwd_f32", pl.x[2].data_ptr(), du.data_ptr(), None, None, B, T, D, 0.0, pl.dxbuf.data_ptr(), None, s)

    def _enqueue_comp_front(self, pl, gather_items: bool = True) -> None:
        """isInC (model_seq.py:89-91): the rows' plain gather, InnerComp's scores and its token group -> pl.x[0] (2T tokens a row:
        [e[g, b, :] | Z[g]]).  gather_items=False: the sequences' rows only."""
        L, s, shp, D = lib(), self.s, pl.shape, self.D
        B = shp.B
        L.call("amid_gather_rows_f32", self.table.data_ptr(), self.n_rows, D, pl.idx_all.data_ptr(), 0, shp.n_idx if gather_items else 2 * shp.Mi,
               pl.xg.data_ptr(), None, s)
        L.call("amid_bert_comp_score_f32", pl.xg.data_ptr(), B, shp.T, D, 0, pl.inc_s.data_ptr(), s)
        L.call("amid_bert_comp_fwd_f32", pl.xg.data_ptr(), pl.inc_s.data_ptr(), self._pp("inc_d{d}.trans_nn.weight"), self._pp("inc_d{d}.trans_nn.bias"),
               self._pp("inc_d{d}.trans_bs.weight"), self._pp("inc_d{d}.trans_bs.bias"), self.inc_threshold, 0, B, shp.T, D, pl.inc_gate.data_ptr(),
               pl.inc_S.data_ptr(), pl.inc_Z.data_ptr(), pl.inc_sw.data_ptr(), pl.x[0].data_ptr(), s)

    def _gru(self, which: str):
        """Host pointer array (domain 0, domain 1) of weight_ih / weight_hh / bias_ih / bias_hh."""
        return self._pp("gru{d}." + which + "_l0")

    def _enqueue_encoders(self, pl, lf, save: bool) -> None:
        """Input projection + recurrence on pl.x[0] (the gathered rows) -> pl.x[2], over the live list `lf` or (None) every sequence.
        save: the form that stores what the backward reads; both forms give the same bits."""
        L, s, shp, D = lib(), self.s, pl.shape, self.D
        B, T = shp.B, shp.Tenc
        L.call("amid_gru_proj_fwd_f32", pl.x[0].data_ptr(), self._gru("weight_ih"), self._gru("bias_ih"), B, T, D, lf, pl.gi.data_ptr(), s)
        if save:
            L.call("amid_gru_rec_fwd_f32", pl.gi.data_ptr(), self._gru("weight_hh"), self._gru("bias_hh"), B, T, D, lf, pl.x[2].data_ptr(),
                   pl.gates.data_ptr(), pl.ghn.data_ptr(), pl.hprev.data_ptr(), s)
        else:
            L.call("amid_gru_rec_fwd_infer_f32", pl.gi.data_ptr(), self._gru("weight_hh"), self._gru("bias_hh"), B, T, D, lf, pl.x[2].data_ptr(), s)

    def enqueue_forward(self, pl: GruPlan, train: bool, with_loss: bool, sum_loss: bool = True) -> None:
        L, s, shp, D = lib(), self.s, pl.shape, self.D
        B, T, NI = shp.B, shp.Tenc, shp.NI
        # the train step's own loss reads only the sequence (domain_id[b], b) of every sample (engine._enqueue_fwd_bwd): with live_fwd the
        # forward encodes nothing else
        lv = self._live_list(pl)
        lf = lv if (lv is not None and getattr(self, "_live_fwd", False)) else None
        if lv is not None and not getattr(pl, "live_packed", False):
            L.call("amid_live_list_i32", pl.domain.data_ptr(), B, pl.live.data_ptr(), s)
        if self.inc_bs:
            self._enqueue_comp_front(pl)
        else:
            self._enqueue_k1(pl, None, None, None, 0, 0.0, lf)      # plain gather: no positional table, no embedding dropout, no "== 0" mask
        self._enqueue_encoders(pl, lf, save=pl.need_grad)
        items = pl.xg.data_ptr() + 4 * 2 * shp.Mi * D
        if self._listwise_fwd(pl, with_loss, sum_loss):
            return
        if (self.dr or self.itc_bs) and getattr(self, "_fuse_scorers", False) and with_loss and not sum_loss:
            self._enqueue_user_vectors(pl)           # train step: the scorers run as ONE forward + loss + backward launch in enqueue_backward
            return
        if self.dr:                                  # three heads (model_seq.py:106-110) on the same user vectors
            self._enqueue_head_dr_fwd(pl, items, with_loss)
            return
        if self.itc_bs:
            self._enqueue_head_itc_fwd(pl, items, with_loss)
            if with_loss and sum_loss:
                L.call("amid_sum_vector_f32", pl.loss_part.data_ptr(), B, pl.loss.data_ptr(), s)
            return
        if getattr(self, "_fuse_head", False) and with_loss and not sum_loss:
            return                                   # train step: the head runs as ONE forward + backward launch in enqueue_backward
        L.call_named("amid_head_fwd_f32", self._scorer(), x=pl.x[2].data_ptr(), ln_w=None, ln_b=None, items=items,
                     labels=pl.labels.data_ptr() if with_loss else None, domain_id=pl.domain.data_ptr() if with_loss else None, B=B, T=T, NI=NI,
                     D=D, hid=self.hid, eps=0.0, u=pl.u.data_ptr(), p1=pl.p1.data_ptr(), p2=pl.p2.data_ptr(),
                     dp1=pl.dp1.data_ptr() if with_loss else None, dp2=pl.dp2.data_ptr() if with_loss else None,
                     loss_part=pl.loss_part.data_ptr() if with_loss else None, stream=s)
        if with_loss and sum_loss:
            L.call("amid_sum_vector_f32", pl.loss_part.data_ptr(), B, pl.loss.data_ptr(), s)

    def enqueue_backward(self, pl: GruPlan, train: bool) -> None:
        L, s, shp, D = lib(), self.s, pl.shape, self.D
        B, T, NI, M = shp.B, shp.Tenc, shp.NI, shp.M
        fp = self.dense
        items = pl.xg.data_ptr() + 4 * 2 * shp.Mi * D
        ditems = pl.dxg.data_ptr() + 4 * 2 * shp.Mi * D
        if self._listwise_bwd(pl, items, ditems, None, None, 0):
            pass
        elif (self.dr or self.itc_bs) and getattr(self, "_fuse_scorers", False):
            self._enqueue_scorers_fused(pl, items, ditems, None, None, 0)
            self._enqueue_user_vectors_bwd(pl)
        elif self.dr:
            self._enqueue_head_dr_bwd(pl, items, ditems)
        elif self.itc_bs:
            self._enqueue_head_itc_bwd(pl, items, ditems)
        elif getattr(self, "_fuse_head", False):
            own = getattr(self, "_live_fwd", False) and self._live_list(pl) is not None      # only the own-domain sequences were encoded
            L.call("amid_head_fwd_bwd_own_f32" if own else "amid_head_fwd_bwd_f32", pl.x[2].data_ptr(), None, None, items, fp.ptr("predictModule.fc.0.weight"),
                   fp.ptr("predictModule.fc.0.bias"), fp.ptr("predictModule.fc.2.weight"), fp.ptr("predictModule.fc.2.bias"),
                   pl.labels.data_ptr(), pl.domain.data_ptr(), B, T, NI, D, self.hid, 0.0, pl.u.data_ptr(), pl.p1.data_ptr(), pl.p2.data_ptr(),
                   pl.dp1.data_ptr(), pl.dp2.data_ptr(), pl.loss_part.data_ptr(), pl.dxbuf.data_ptr(), ditems, None, pl.sc_part.data_ptr(),
                   None, None, 0, s)
        else:
            L.call_named("amid_head_bwd_f32", self._scorer(), x=pl.x[2].data_ptr(), ln_w=None, u=pl.u.data_ptr(), items=items, p1=pl.p1.data_ptr(),
                         p2=pl.p2.data_ptr(), dp1=pl.dp1.data_ptr(), dp2=pl.dp2.data_ptr(), B=B, T=T, NI=NI, D=D, hid=self.hid, eps=0.0,
                         dx=pl.dxbuf.data_ptr(), ditems=ditems, ln_part=None, sc_part=pl.sc_part.data_ptr(), tr_src=None, tr_dst=None, n_tr=0,
                         stream=s)
        # the train step's own backward walks the LIVE sequences only (the loss sends no gradient into the other domain's encoder of a
        # sample); their rows of dgi / dgh / dxg are zero-filled: the weight gradients may walk, and the segment reduce reads, every row.
        # InterComp mixes the rows' user vectors (_own_domain_only is off: no list); InnerComp in front of the encoders reads the gradient of
        # EVERY encoder-input row: all rows then
        lv = None if self.inc_bs else self._live_list(pl)
        L.call("amid_gru_rec_bwd_f32", pl.dxbuf.data_ptr(), pl.gates.data_ptr(), pl.ghn.data_ptr(), pl.hprev.data_ptr(), self._gru("weight_hh"),
               B, T, D, lv, 1, pl.dgi.data_ptr(), pl.dgh.data_ptr(), s)
        # dW_ih = dGi^T X, dW_hh = dGh^T H_prev as six 128 x 128 tiles per domain with split partials; the biases are their column sums
        dy = [pl.dgi.data_ptr() + 4 * c * D for c in range(3)] + [pl.dgh.data_ptr() + 4 * c * D for c in range(3)]
        xx = [pl.x[0].data_ptr()] * 3 + [pl.hprev.data_ptr()] * 3
        ia = lambda v: (ctypes.c_int * N_ENT)(*v)      # noqa: E731
        L.call("amid_bert_wgrad_mode_f32", ptr_array(dy), ptr_array(xx), ia([3 * D] * N_ENT), ia([D] * N_ENT), ia([D] * N_ENT), ia(range(N_ENT)),
               ia([0] * N_ENT), N_ENT, M, pl.splits, pl.w_part.data_ptr(), pl.b_part.data_ptr(), self._own_rows(pl) if lv is not None else None,
               B, T, 0, s)
        L.call("amid_gru_dx_f32", pl.dgi.data_ptr(), self._gru("weight_ih"), B, T, D, lv, 1, (pl.dx0 if self.inc_bs else pl.dxg).data_ptr(), s)
        if self.inc_bs:      # InnerComp's parameter gradients (written whole); the rows' own halves + their share of dZ -> the table-row gradients
            G = self.dense.grad
            L.call("amid_bert_comp_bwd_f32", pl.xg.data_ptr(), pl.dx0.data_ptr(), pl.inc_gate.data_ptr(), pl.inc_S.data_ptr(), pl.inc_sw.data_ptr(),
                   self._pp("inc_d{d}.trans_nn.weight"), self._pp("inc_d{d}.trans_nn.bias"), self._pp("inc_d{d}.trans_bs.weight"), 0, B, shp.T, D,
                   pl.inc_dZ.data_ptr(), pl.inc_dS.data_ptr(), pl.inc_rows.data_ptr(), self._pp("inc_d{d}.trans_nn.weight", G),
                   self._pp("inc_d{d}.trans_nn.bias", G), self._pp("inc_d{d}.trans_bs.weight", G), self._pp("inc_d{d}.trans_bs.bias", G),
                   pl.dxg.data_ptr(), s)
        self._enqueue_grad_tail(pl)

    # ------------------------------------------------------------------ evaluation: test(), train_sr.py:31-128 (engine.enqueue_eval)
    # The batch is amid_pack_indices_live (index marshal + live list), the live sequences' rows (amid_embed_fwd_live_f32), the projection and
    # the inference recurrence over the live list, amid_eval_head_f32 with null LayerNorm pointers (the plain mean over time; the scorer over
    # the gathered candidates, masked BCE, both ranks): five launches, one graph replay.  Every live row of pl.x[2] has the bits of
    # enqueue_forward(train=False): the same kernels, whose arithmetic does not depend on a sequence's tile or slot.
    #   isInC:  amid_gather_rows_f32 over the sequences' rows + the comp score / token-group launches in place of the live gather (the group
    #           is built from every row of the batch), then the recurrence at 2T over the live list.
    #   isItC:  both domains of every sample (a plain gather, a null live list), amid_itc_pairmax_raw_f32 with mix=False and
    #           amid_eval_head_u_f32 with the mix folded in (32 <= B <= 256; amid_itc_mix_fwd_f32 in front otherwise): engine.enqueue_eval.
    #   isDR:   amid_lnmean_fwd_f32 + amid_eval_head_u_f32 on predictModule (predict_ips / predict_gfunc are not evaluated).
    def eval_fused_ok(self, pl) -> bool:
        if not self.EVAL_FUSED or not getattr(pl, "strip", False) or self.input_pool(pl) is not None:
            return False
        return bool(self.D % 32 == 0 and self.D <= 128 and 0 < self.hid <= 64 and self.hid % 4 == 0)      # the head's limits (amid_eval_head_f32)

    def _eval_through_forward(self) -> bool:
        return False

    def _eval_last_ln(self):
        return dict(ln_w=None, ln_b=None, eps=0.0)

    def _enqueue_eval_images(self, pl) -> None:
        pass                     # (no derived weight images: the kernels read the parameters)

    def _enqueue_eval_encoders(self, pl, build_images: bool) -> None:
        """The own-domain sequences' rows and the inference forward of an evaluation batch, up to pl.x[2] (the live rows only)."""
        L, shp = lib(), pl.shape
        lf = None if self.itc_bs else pl.live.data_ptr()      # isItC: the pair-max reads both domains' rows of every sample
        if self.inc_bs:          # the token group is built from every row of the batch, whatever the encoders then step through
            self._enqueue_comp_front(pl, gather_items=False)
        elif lf is None:
            L.call("amid_gather_rows_f32", self.table.data_ptr(), self.n_rows, self.D, pl.idx_all.data_ptr(), 0, 2 * shp.Mi, pl.xg.data_ptr(), None, self.s)
        else:
            L.call("amid_embed_fwd_live_f32", self.table.data_ptr(), pl.idx_all.data_ptr(), None, None, shp.B, shp.Tenc, self.D, 0, pl.xg.data_ptr(),
                   None, self.step_state.data_ptr(), 0, 0.0, lf, self.s)
        self._enqueue_encoders(pl, lf, save=False)
