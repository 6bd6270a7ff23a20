"""Drop-in ``nn.Module`` surface of the reference's ``model_seq.py`` for the MI355X hot path.

Same class names, constructor signatures, ``forward`` signatures and ``state_dict`` keys as the
reference; the arithmetic runs in the hand-written HIP kernels of
``libamid_hip.so`` (there is no PyTorch fallback: without the library, construction raises).

  SASRec(user_length, user_emb_dim, item_length, item_emb_dim, seq_len, hid_dim, bs,
         isInC, isItC, threshold1, threshold2, isDR=False)          model_seq.py:391
      forward(u_node, i_node, neg_samples, seq_d1, seq_d2, long_tail_mask_d1, long_tail_mask_d2,
              isTrain=True) -> (logits_d1, logits_d2)                 model_seq.py:416
  BERT4Rec(same arguments)                                            model_seq.py:250
      forward(same arguments) -> (logits_d1, logits_d2)               model_seq.py:277
  embItemLayerEnhance(item_length, emb_dim)                           model_seq.py:23
  predictModule(emb_dim, hid_dim)                                     model_seq.py:33
  Log2feats(user_length, user_emb_dim, item_length, item_emb_dim, seq_len, hid_dim)   model_seq.py:332

As in the reference, ``u_node``, both ``long_tail_mask_*``, ``isTrain``, ``user_length`` and ``bs``
are accepted and ignored; dropout follows ``module.training``.  Two ways to train:

  reference loop   ``opt = torch.optim.Adam(model.parameters(), lr)``; ``loss.backward(); opt.step()``
                   (train_sr.py:213-215) works unchanged: backward runs the HIP kernels and hands autograd
                   the gradients (the table gradient is materialised densely for torch's optimizer);
                   with ``amid_amd.optim.Adam`` in place of ``torch.optim.Adam`` the table gradient stays the step's
                   unique rows and ``step()`` is the engine's one-launch dense-equivalent lazy Adam (optim.py);
  fused step       ``model.train_step(batch)`` = forward + masked BCE + backward + dense-equivalent lazy
                   Adam as one hipGraph replay -- what ``train_sr.py`` of this repo and ``bench.py`` use.

Out of scope (constructor kept for import parity, ``forward`` raises): embUserLayerEnhance (dead code in the reference).  GRU4Rec is built
in ``amid_amd.model_gru``; the ``GRU4Rec`` of this module is a stub that raises and names that class.  BERT4Rec(isInC=True) / (isItC=True) -- the comp module in
FRONT of the encoders, model_seq.py:283-294 -- are built (the reference itself fails with both flags).
SASRec(isItC=True, isDR=True) -- InterComp after the encoders + the doubly-robust heads, what run.sh trains through
train_sr_dr.py -- IS built (csrc/intercomp.hip, amid_dr_loss_f32), and so is SASRec(isInC=True) -- InnerComp on the gathered rows
before the encoders, which then run over 2 * seq_len tokens (csrc/innercomp.hip).
"""
from __future__ import annotations

import weakref
from collections import namedtuple
from typing import Dict, Optional

import torch
import torch.nn as nn

from ._lib import lib, ptr_array
from .engine import SASREC_LN_EPS, SasrecEngine
from .engine_bert import Bert4recEngine

# what rank_candidates / rank_candidates_from_vectors return: device tensors, a field not asked for is None
RankedLists = namedtuple("RankedLists", ["ids", "scores", "positions", "list_scores"])
DiverseLists = namedtuple("DiverseLists", ["ids", "scores", "values", "max_sims", "positions"])


def _register_tree(root: nn.Module, dotted: str, param: nn.Parameter) -> None:
    """Register ``param`` under a dotted state_dict name, creating plain container modules on the way."""
    parts = dotted.split(".")
    mod = root
    for p in parts[:-1]:
        if p not in mod._modules:
            mod.add_module(p, nn.Module())
        mod = mod._modules[p]
    mod.register_parameter(parts[-1], param)


def _not_built(what: str, cite: str):
    raise NotImplementedError(
        f"{what} ({cite}) is outside the MI355X hot path built so far (SURVEY.md section 8(f)); the constructor exists for "
        f"signature / state_dict parity only.  There is deliberately no PyTorch fallback.")


# ------------------------------------------------------------------------------------------------
class _SasrecFunction(torch.autograd.Function):
    """Autograd bridge: forward / backward are the HIP launch sequences of SasrecEngine."""

    @staticmethod
    def forward(ctx, model, need_grad, i_node, neg_samples, seq_d1, seq_d2, *params):
        eng: SasrecEngine = model.engine
        B, T = seq_d1.shape
        neg = neg_samples.reshape(B, -1)
        pl = eng.plan(B, T, 1 + neg.shape[1], need_grad=bool(need_grad))
        eng.stream.wait_stream(torch.cuda.current_stream())
        eng.load_batch(pl, i_node, neg, seq_d1, seq_d2)
        loop = model._loop if model._amid_optims else None      # an amid_amd.optim.Adam drives this model (its contract: optim.py)
        if model.training:
            if loop is None or loop["fwd"] == 0:
                eng.enqueue_step_begin()               # fresh dropout counter per training forward
            if loop is not None:
                loop["fwd"] += 1                       # (a second one before step() is refused there: it takes no further bump, so the
                                                       # refusal leaves the lazy rows' stamps consistent)
        eng.enqueue_prepare(pl, sparse=need_grad)
        if need_grad and eng.table_m is not None:
            eng.enqueue_catchup(pl)                    # lazy-Adam rows must be current before they are gathered
        eng.enqueue_forward(pl, train=model.training, with_loss=False)
        torch.cuda.current_stream().wait_stream(eng.stream)
        ctx.model, ctx.pl, ctx.train = model, pl, model.training
        eng.check_index_error(pl)
        outs = (pl.p1, pl.p2) + ((pl.ips1, pl.ips2, pl.g1, pl.g2) if eng.dr else ())      # isDR: model_seq.py:436-440
        return tuple(o.clone() for o in outs)

    @staticmethod
    def backward(ctx, *gouts):
        model, pl = ctx.model, ctx.pl
        eng: SasrecEngine = model.engine
        loop = model._loop if model._amid_optims else None
        if loop is not None and loop["bwd"] >= 1:
            raise RuntimeError("amid_amd.optim.Adam: a second backward() before step() (gradient accumulation) is not supported: one plan "
                               "holds one batch's table rows -- exactly one training-mode forward and backward between two step() calls")
        eng.stream.wait_stream(torch.cuda.current_stream())
        dsts = (pl.dp1, pl.dp2) + ((pl.dips1, pl.dips2, pl.dg1, pl.dg2) if eng.dr else ())
        with torch.cuda.stream(eng.stream):
            for d, g in zip(dsts, gouts):
                if g is None:
                    d.zero_()
                else:
                    d.copy_(g.reshape(d.shape))
        eng.enqueue_backward(pl, train=ctx.train)
        grads = []
        # every dense .grad is its view of the optimizer's flat buffer (what optim.Adam.zero_grad() installs): the engine's dense gradient is
        # added to that buffer in ONE launch and autograd is handed nothing to accumulate -- no copy and no addition per parameter
        if loop is not None and all(p.grad is not None and p.grad.data_ptr() == v.data_ptr() for p, v in zip(model._amid_dense_params, model._amid_gviews)):
            with torch.cuda.stream(eng.stream):
                model._amid_gflat.add_(eng.dense.grad)
            torch.cuda.current_stream().wait_stream(eng.stream)
            model._last_plan = pl
            loop["bwd"] += 1
            return (None,) * (6 + len(model._param_names))
        with torch.cuda.stream(eng.stream):
            for name in model._param_names:
                if name == "item_emb_layer.emb_item.weight":
                    if model.fused_optimizer or loop is not None:
                        grads.append(None)             # rows stay in pl.uniq_ids / pl.uniq_grad for the lazy Adam
                    else:
                        U = int(pl.n_uniq.item())
                        dense = torch.zeros_like(eng.table)
                        dense.index_copy_(0, pl.uniq_ids[:U].long(), pl.uniq_grad[:U])
                        grads.append(dense)
                else:
                    grads.append(eng.dense.view(name, eng.dense.grad).clone())
        torch.cuda.current_stream().wait_stream(eng.stream)
        model._last_plan = pl
        if loop is not None:
            loop["bwd"] += 1
        return (None, None, None, None, None, None, *grads)


class SASRec(nn.Module):
    """model_seq.py:390-443 on the HIP engine (isInC / isItC either way: with either every batch must hold exactly `bs` rows,
    as in the reference where trans_bs is Linear(bs, 1) over the batch, and state_dict gains inc_d{1,2}.* / itc_d{1,2}.*; with
    isInC the encoders run over 2 * seq_len tokens and pos_emb has 2 * seq_len rows, :398-401; isDR either way:
    with it forward returns six outputs -- logits, ips, gfunc per domain, :436-440 -- and state_dict gains predict_ips.*,
    predict_gfunc.*)."""

    ENGINE_CLS = SasrecEngine
    COMP_IN_FRONT = False        # InterComp after the encoders (model_seq.py:426-431), the configuration run.sh trains

    def __init__(self, user_length, user_emb_dim, item_length, item_emb_dim, seq_len, hid_dim, bs, isInC, isItC, threshold1,
                 threshold2, isDR=False, device: Optional[str] = None, lr: float = 5e-4, seed: int = 0, compute: str = "f32", loss: str = "bce",
                 hard_negs: int = 0, hard_skip: int = 0):
        """Beyond the reference's arguments: device, lr / seed (the fused train_step owns Adam and the dropout counter),
        compute ("f32": exact fp32 matrix products, the default; "bf16": bf16 MFMA operands with fp32 accumulation, SASRec with
        emb_dim 128 only -- BASELINE.json configs[2]) and loss ("bce": the reference's masked BCE, the default; "softmax" / "bpr":
        sampled softmax / BPR of a fused train step over the row's positive, column 0, and its sampled negatives -- refused with
        isDR, isInC, compute "bf16" and data parallel; evaluation and the autograd path are unchanged) with hard_negs / hard_skip (H > 0:
        the step trains on the H of the sampled negatives that the current model ranks hard_skip .. hard_skip + H - 1 by logit, DESIGN.md
        section 18; needs loss "softmax" / "bpr")."""
        super().__init__()
        if isInC and isItC and self.COMP_IN_FRONT:
            raise ValueError("BERT4Rec(isInC=True, isItC=True): the reference itself fails on this combination (its key mask keeps 2T "
                             "keys for 4T tokens, model_seq.py:294); pick one")
        if user_emb_dim != item_emb_dim:
            raise ValueError("the reference feeds item rows into encoders built with user_emb_dim: the two must be equal")
        lib()                                                   # fail loudly without libamid_hip.so
        self.user_emb_dim = user_emb_dim
        self.isInC, self.isItC, self.isDR = isInC, isItC, isDR
        dev = device or ("cuda:%d" % torch.cuda.current_device())
        kw = {}
        if self.COMP_IN_FRONT:          # BERT4Rec: either module runs on the gathered rows, before the encoders (:283-294)
            if isInC or isItC:
                kw.update(comp="inc" if isInC else "itc", comp_bs=bs, comp_threshold=threshold1 if isInC else threshold2)
        else:
            if isItC:
                kw.update(itc_bs=bs, itc_threshold=threshold2)
            if isInC:
                kw.update(inc_bs=bs, inc_threshold=threshold1)
        if isDR:
            kw["dr"] = True
        if compute != "f32":
            kw["compute"] = compute
        if loss != "bce":
            kw["loss"] = loss
        if hard_negs or hard_skip:
            kw.update(hard_negs=hard_negs, hard_skip=hard_skip)
        self.engine = self.ENGINE_CLS(item_length, item_emb_dim, seq_len, hid_dim, device=dev, lr=lr, seed=seed, **kw)
        eng = self.engine
        self._param_names = ["item_emb_layer.emb_item.weight"] + list(eng.dense.slots)
        self._init_reference_defaults(seed)
        _register_tree(self, "item_emb_layer.emb_item.weight", nn.Parameter(eng.table))
        for name in eng.dense.slots:
            _register_tree(self, name, nn.Parameter(eng.dense.view(name)))
        self.fused_optimizer = False            # set by train_step(): table gradient stays sparse, Adam runs in HIP
        self._last_plan = None
        # amid_amd.optim.Adam finds the model from its parameters (a weak reference on each) and binds itself here; _loop counts the
        # training-mode forwards and the backwards since the last step()
        self._amid_optims: list = []
        self._loop = {"fwd": 0, "bwd": 0}
        me = weakref.ref(self)
        for p in self.parameters():
            p._amid_owner = me

    def _init_reference_defaults(self, seed: int) -> None:
        """Same initial distributions as the reference's modules (nn.Embedding N(0,1); nn.Linear / Conv1d /
        MultiheadAttention defaults; LayerNorm 1/0), drawn from a private generator."""
        eng = self.engine
        g = torch.Generator(device="cpu").manual_seed(seed)
        D, hid = eng.D, eng.hid
        with torch.no_grad():
            eng.table.copy_(torch.randn(eng.n_rows, D, generator=g))
            for name in eng.dense.slots:
                v = eng.dense.view(name)
                if name.endswith("pos_emb.weight"):
                    v.copy_(torch.randn(v.shape, generator=g))
                elif "layernorm" in name:
                    v.fill_(1.0 if name.endswith("weight") else 0.0)
                elif name.endswith("norm.a_2") or name.endswith("norm.b_2"):      # BERT4Rec LayerNorm, model_seq.py:119-120
                    v.fill_(1.0 if name.endswith("a_2") else 0.0)
                elif name.endswith("in_proj_weight"):          # xavier_uniform_ (nn.MultiheadAttention._reset_parameters)
                    a = (6.0 / (3 * D + D)) ** 0.5
                    v.copy_((torch.rand(v.shape, generator=g) * 2 - 1) * a)
                elif name.endswith("in_proj_bias") or name.endswith("out_proj.bias"):
                    v.zero_()
                else:                                          # kaiming_uniform_(a=sqrt(5)) => U(-1/sqrt(fan_in), 1/sqrt(fan_in))
                    fan_in = {"predictModule.fc.0.weight": 2 * D, "predictModule.fc.0.bias": 2 * D, "predictModule.fc.2.weight": hid,
                              "predictModule.fc.2.bias": hid}.get(name, 4 * D if ".feed_forward.w_2." in name else D)
                    if ".trans_bs." in name:                   # Inter/InnerComp's Linear(bs, 1) over the batch (model_seq.py:480, :457)
                        fan_in = eng.itc_bs or eng.inc_bs
                    elif name.startswith(("predict_ips.fc.0", "predict_gfunc.fc.0")):
                        fan_in = 2 * D
                    elif name.startswith(("predict_ips.fc.2", "predict_gfunc.fc.2")):
                        fan_in = hid
                    a = 1.0 / fan_in ** 0.5
                    v.copy_((torch.rand(v.shape, generator=g) * 2 - 1) * a)
        torch.cuda.synchronize(eng.device)

    # -- reference forward ---------------------------------------------------------------------
    def forward(self, u_node, i_node, neg_samples, seq_d1, seq_d2, long_tail_mask_d1, long_tail_mask_d2, isTrain=True):
        if not self.training and self.engine.table_m is not None:
            self.engine.flush_table()               # rows with pending zero-gradient Adam steps must be current for eval
        params = [self.get_parameter(n) for n in self._param_names]
        need_grad = torch.is_grad_enabled() and any(p.requires_grad for p in params)
        outs = _SasrecFunction.apply(self, need_grad, i_node, neg_samples, seq_d1, seq_d2, *params)
        return tuple(o.squeeze() for o in outs)        # model_seq.py:54 ; isDR: six outputs (:436-440)

    # -- fused fast path -------------------------------------------------------------------------
    def train_step(self, i_node, neg_samples, seq_d1, seq_d2, labels, domain_id, use_graph: bool = True, exchange=None,
                   ob_label=None, dr_objective: int = 0) -> torch.Tensor:
        """train_sr.py:190-217 as one launch sequence (one hipGraph replay once captured).  Returns the loss (device scalar;
        under data parallelism the mean over THIS rank's shard).  exchange: an amid_amd.dist.SparseDenseExchange for
        data-parallel training (one process per GPU): local gradients, one dense all-reduce + sparse all-gather, Adam.
        isDR models: dr_objective 0 = loss_cls + dr_e_w * loss_dr_e (train_sr_dr.py:216-224), 1 = loss_dr_r with ob_label
        (:392-398); returns the three-element tensor (loss_cls, loss_dr_e, loss_dr_r) of this batch.  Pick the Adam state with
        engine.select_optimizer() (the reference alternates two optimizers)."""
        eng = self.engine
        if self._loop["fwd"]:
            raise RuntimeError("train_step() between a training-mode forward and the step() of an amid_amd.optim.Adam: finish that step first")
        self.fused_optimizer = True
        B, T = seq_d1.shape
        neg = neg_samples.reshape(B, -1)
        pl = eng.plan(B, T, 1 + neg.shape[1], need_grad=True)
        eng.stream.wait_stream(torch.cuda.current_stream())
        if eng.dr:
            eng.dr_mode = int(dr_objective)
            if ob_label is None:
                if eng.dr_mode == 1:
                    raise ValueError("dr_objective 1 (loss_dr_r) needs ob_label (train_sr_dr.py:372)")
                ob_label = torch.zeros(B, dtype=torch.int64, device=seq_d1.device)
        eng.load_batch(pl, i_node, neg, seq_d1, seq_d2, labels, domain_id, ob_label if eng.dr else None)
        if exchange is not None and exchange.world > 1:
            # (isItC / isInC: collectives inside the step -- no local graph; train_step_dp replays graph segments once it knows a bound)
            if use_graph and not (eng.itc_bs or eng.inc_bs) and not eng.has_local_graph(pl):
                eng.capture_local_grads(pl)
            eng.train_step_dp(pl, exchange, use_graph=use_graph)
        elif use_graph:
            if not eng.has_graph(pl):
                eng.capture_train_step(pl)
            eng.replay_train_step(pl)
        else:
            eng.enqueue_train_step(pl)
        torch.cuda.current_stream().wait_stream(eng.stream)
        self._last_plan = pl
        return pl.dr_losses if eng.dr else pl.loss

    def begin_epoch_pool(self, ep: Dict[str, torch.Tensor], exchange=None, dr_objective: int = 0) -> int:
        """Make a whole epoch resident in HBM (ep = DeviceBatches.epoch_tensors()): the batches are packed into one
        [n_batches, words] tensor and every following pool_step() consumes the next one, picked on the device by the step counter
        -- no per-step input copies or host tensor work (train_sr.py:185-199 builds and moves each batch inside the loop).
        Returns the number of batches.  Under data parallelism the world's largest per-step unique-row count of the epoch is reduced
        here, once, so the sparse exchange of every step runs without a device -> host sync."""
        eng = self.engine
        if eng.dr:
            eng.dr_mode = int(dr_objective)          # isDR: a pool belongs to the (Adam state, objective) selected now
        nb, B, T = ep["seq_d1"].shape
        neg = ep["neg_samples"].reshape(nb, B, -1)
        pl = eng.plan(B, T, 1 + neg.shape[2], need_grad=True)
        eng.stream.wait_stream(torch.cuda.current_stream())
        pool = eng.pack_epoch(pl, ep["i_node"], neg, ep["seq_d1"], ep["seq_d2"], ep["label"], ep["domain_id"], ep.get("ob_label") if eng.dr else None)
        self._pool_umax = None
        if exchange is not None and exchange.world > 1:
            idx = torch.cat((ep["i_node"].reshape(nb, -1), neg.reshape(nb, -1), ep["seq_d1"].reshape(nb, -1), ep["seq_d2"].reshape(nb, -1)), 1)
            srt = torch.sort(idx, dim=1).values
            cnt = ((srt[:, 1:] != srt[:, :-1]).sum(1) + 1).max().reshape(1)
            exchange.all_reduce_max(cnt)
            self._pool_umax = (int(cnt.item()) + 255) // 256 * 256          # one bucketed bound per epoch: the exchange's graph pair is reused
        torch.cuda.current_stream().synchronize()
        if not eng.refill_input_pool(pl, pool):            # same shape, step on a pool boundary: the captured graphs stay valid
            eng.set_input_pool(pl, pool)
        self._pool_plan = pl
        self.fused_optimizer = True
        return nb

    def pool_step(self, use_graph: bool = True, exchange=None, dr_objective: int = 0, n_steps: int = 1) -> torch.Tensor:
        """One train step on the next batch of the pool installed by begin_epoch_pool(); returns what train_step() returns.
        n_steps > 1 (single GPU, graphs): that many consecutive steps as ONE replayed graph (the caller sees the last step's loss)."""
        eng, pl = self.engine, self._pool_plan
        if eng.dr:
            eng.dr_mode = int(dr_objective)
        if n_steps > 1:
            if not use_graph or (exchange is not None and exchange.world > 1):
                raise ValueError("several steps per call need graph replay on a single GPU")
            if (eng._graph_key(), n_steps) not in getattr(pl, "graphs_n", {}):
                eng.capture_train_steps(pl, n_steps)
            eng.replay_train_steps(pl, n_steps)
        elif exchange is not None and exchange.world > 1:
            # (isItC / isInC: collectives inside the step -- no local graph; with the epoch's bound train_step_dp replays graph SEGMENTS
            # cut at those collectives, engine._coll)
            if use_graph and not (eng.itc_bs or eng.inc_bs) and not eng.has_local_graph(pl):
                eng.capture_local_grads(pl)
            eng.train_step_dp(pl, exchange, use_graph=use_graph, umax=self._pool_umax)
        elif use_graph:
            if not eng.has_graph(pl):
                eng.capture_train_step(pl)
            eng.replay_train_step(pl)
        else:
            eng.enqueue_train_step(pl)
        self._last_plan = pl
        return pl.dr_losses if eng.dr else pl.loss

    def eval_ranks(self, ep: Dict[str, torch.Tensor], fix_value: float, use_graph: bool = True) -> Optional[Dict[str, torch.Tensor]]:
        """test()'s arithmetic (train_sr.py:31-128) over a whole evaluation set resident in HBM (ep = DeviceBatches.epoch_tensors()):
        per batch the eval-mode forward of every sample's OWN domain sequence, its 1 + neg_nums scores, the masked BCE mean (:63-64) and
        the positive's rank with and without fix_value (:114-115; utils.py:21-40, :296-297) -- three launches replayed as one graph
        (SasrecEngine.enqueue_eval; isDR / isItC / isInC models: the launches their forward forms the user vectors with, both domains'
        sequences where a comp module needs them, and the same scorer launch).  Returns device tensors rank [n, B], rank_raw [n, B]
        (int32) and loss [n], or None when this model evaluates through forward() (shapes the engine's evaluation does not cover -- for
        BERT4Rec: more than 64 encoder tokens, a row-tile plan --, a comp model whose batch is not its bs rows: forward() then raises what it
        always raised).  BERT4Rec (plain, isDR, isInC, isItC) runs the same batch on its own encoders: one launch for both blocks, or the
        strips staged (Bert4recEngine._enqueue_eval_encoders)."""
        eng = self.engine
        nb, B, T = ep["seq_d1"].shape
        neg = ep["neg_samples"].reshape(nb, B, -1)
        pl = eng.plan(B, T, 1 + neg.shape[2], need_grad=False)
        if not eng.eval_fused_ok(pl):
            return None
        eng.stream.wait_stream(torch.cuda.current_stream())
        packed = eng.pack_epoch(pl, ep["i_node"], neg, ep["seq_d1"], ep["seq_d2"], ep["label"], ep["domain_id"])
        eng.stream.wait_stream(torch.cuda.current_stream())
        out = eng.eval_epoch(pl, packed, fix_value, with_loss=True, use_graph=use_graph)
        torch.cuda.current_stream().wait_stream(eng.stream)
        eng.check_index_error(pl)
        return {"rank": out[:, :B], "rank_raw": out[:, B:2 * B], "loss": out[:, 2 * B:].view(torch.float32).sum(1)}

    def _check_comp_batch(self, B: int) -> None:
        eng = self.engine
        bs = eng.itc_bs or eng.inc_bs or getattr(eng, "comp_bs", 0)
        if bs and B != bs:
            raise ValueError(f"the batch must hold exactly bs = {bs} rows (trans_bs is Linear(bs, 1) over the batch), got {B}")

    @torch.no_grad()
    def full_ranks(self, ep: Dict[str, torch.Tensor], batches, fix_value: float) -> Dict[str, torch.Tensor]:
        """The positive's rank against EVERY candidate its sampled negatives could have been (the domain's pool minus the row's own items,
        dataset_seq.py:188 / :206) instead of neg_nums of them, by test()'s rule (train_sr.py:114-115): ep = batches.epoch_tensors() of an
        unshuffled DeviceBatches, whose pools and own sets are used.  Returns device tensors rank / rank_raw [n, B] (int32), shaped like
        eval_ranks'; the user vectors are the ones the sampled evaluation scores."""
        eng = self.engine
        if getattr(batches, "shuffle", True) or not hasattr(batches, "own"):
            raise ValueError("full_ranks needs the evaluation's unshuffled DeviceBatches (its row order gives the rows' own item sets)")
        nb, B, T = ep["seq_d1"].shape
        self._check_comp_batch(B)
        if eng.table_m is not None:
            eng.flush_table()
        neg = ep["neg_samples"].reshape(nb, B, -1)
        pl = eng.plan(B, T, 1 + neg.shape[2], need_grad=False)
        dev = eng.device
        rank = torch.empty(nb, B, dtype=torch.int32, device=dev)
        rank_raw = torch.empty(nb, B, dtype=torch.int32, device=dev)
        # the dataset rows of batch i (DeviceBatches.__iter__ without shuffling): (i * world + rank) * bs + 0 .. bs - 1
        rows = ((torch.arange(nb, device=dev) * batches.world + batches.rank) * B).unsqueeze(1) + torch.arange(B, device=dev)
        rows = rows.to(torch.int32)
        pools = (batches.pool[0], batches.pool[1])
        eng.stream.wait_stream(torch.cuda.current_stream())
        for i in range(nb):
            eng.load_batch(pl, ep["i_node"][i], neg[i], ep["seq_d1"][i], ep["seq_d2"][i], ep["label"], ep["domain_id"][i])
            eng.enqueue_full_rank(pl, ep["i_node"][i], ep["domain_id"][i], pools, batches.own, batches.own_off, rows[i], fix_value, rank[i],
                                  rank_raw[i])
        torch.cuda.current_stream().wait_stream(eng.stream)
        eng.check_index_error(pl)
        return {"rank": rank, "rank_raw": rank_raw}

    @torch.no_grad()
    def recommend(self, seq_d1, seq_d2, domain_id, k: int = 10, pool=None, exclude_history: bool = True):
        """The k items the model scores highest for each user (rows of seq_d1 / seq_d2 [B, T], domain_id [B]: the domain to recommend in),
        best first, ties to the lower id.  pool: the candidate item ids -- None = every row of the table, a tensor = the same pool for both
        domains, a pair = (domain 0's, domain 1's).  exclude_history drops the ids of the row's own-domain sequence.  Returns (ids [B, k]
        int64, scores [B, k] float32) on the device; a row with fewer than k candidates is padded with id -1 and score -inf."""
        eng = self.engine
        dev = eng.device
        seq_d1 = torch.as_tensor(seq_d1).to(dev, torch.int64).contiguous()
        seq_d2 = torch.as_tensor(seq_d2).to(dev, torch.int64).contiguous()
        B, T = seq_d1.shape
        dom = torch.as_tensor(domain_id).to(dev, torch.int64).reshape(B).contiguous()
        self._check_comp_batch(B)
        if not 1 <= int(k) <= 256:
            raise ValueError(f"k must be in 1..256, got {k}")
        if eng.table_m is not None:
            eng.flush_table()
        if pool is None:
            p = torch.arange(eng.n_rows, dtype=torch.int64, device=dev)
            pools = (p, p)
        elif isinstance(pool, (tuple, list)):
            pools = tuple(torch.unique(torch.as_tensor(q).to(dev, torch.int64)) for q in pool)
        else:
            p = torch.unique(torch.as_tensor(pool).to(dev, torch.int64))
            pools = (p, p)
        if min(int(q.numel()) for q in pools) < 1:
            raise ValueError("recommend: an empty candidate pool")
        # own(b): the sorted unique ids of the row's own-domain sequence, as one CSR list
        srt = torch.sort(torch.where(dom.unsqueeze(1) != 0, seq_d2, seq_d1), dim=1).values
        keep = torch.ones_like(srt, dtype=torch.bool)
        keep[:, 1:] = srt[:, 1:] != srt[:, :-1]
        own = srt[keep].contiguous()
        own_off = torch.zeros(B + 1, dtype=torch.int32, device=dev)
        own_off[1:] = torch.cumsum(keep.sum(1), 0).to(torch.int32)
        rows = torch.arange(B, dtype=torch.int32, device=dev)
        zero = torch.zeros(B, dtype=torch.int64, device=dev)
        label = torch.zeros(B, 2, device=dev)
        ids = torch.empty(B, int(k), dtype=torch.int64, device=dev)
        scores = torch.empty(B, int(k), dtype=torch.float32, device=dev)
        pl = eng.plan(B, T, 2, need_grad=False)
        eng.stream.wait_stream(torch.cuda.current_stream())
        eng.load_batch(pl, zero, zero.view(B, 1), seq_d1, seq_d2, label, dom)
        eng.enqueue_topk(pl, dom, pools, own, own_off, rows, int(k), exclude_history, ids, scores)
        torch.cuda.current_stream().wait_stream(eng.stream)
        eng.check_index_error(pl)
        return ids, scores

    def _candidate_pools(self, pool):
        """recommend()'s `pool` argument as (domain 0's, domain 1's) sorted unique int64 device tensors.  The whole table (None) is one
        tensor for the life of the model, and a pool that is already such a tensor is passed through, so that recommend_all's captured
        graphs, which hold the pools' addresses, survive from call to call."""
        eng = self.engine
        dev = eng.device
        if pool is None:
            if getattr(self, "_all_rows", None) is None:
                self._all_rows = torch.arange(eng.n_rows, dtype=torch.int64, device=dev)
            return (self._all_rows, self._all_rows)

        def one(q):
            if isinstance(q, torch.Tensor) and q.device == dev and q.dtype == torch.int64 and q.dim() == 1 and q.is_contiguous() \
                    and (q.numel() < 2 or bool((q[1:] > q[:-1]).all())):
                return q
            return torch.unique(torch.as_tensor(q).to(dev, torch.int64))
        if isinstance(pool, (tuple, list)):
            pools = tuple(one(q) for q in pool)
            if len(pools) != 2:
                raise ValueError("recommend_all: pool is None, one tensor of item ids, or a pair (domain 0's, domain 1's)")
            return pools
        p = one(pool)
        return (p, p)

    @torch.no_grad()
    def recommend_all(self, users: Dict[str, torch.Tensor], k: int = 10, pool=None, exclude_history: bool = True, use_graph: bool = True):
        """recommend() for every batch of a dataset: users = {"seq_d1", "seq_d2": [n, B, T], "domain_id": [n, B]} (what
        DeviceBatches.epoch_tensors() gives fits; other keys are ignored), pool / k / exclude_history as in recommend().  Returns
        (ids [n, B, k] int64, scores [n, B, k] float32) on the device: batch i's rows are recommend()'s for the same batch, bit for bit
        (ordering, ties to the lower id, -1 / -inf padding).  The weights do not change inside the call, so the candidates' item halves
        are formed once, the history sets come from the sequences on the device, and a batch is one device copy of its packed image and
        one graph replay (SasrecEngine.topk_epoch; use_graph=False: the same launches, eagerly)."""
        eng = self.engine
        dev = eng.device
        seq_d1 = torch.as_tensor(users["seq_d1"]).to(dev, torch.int64)
        seq_d2 = torch.as_tensor(users["seq_d2"]).to(dev, torch.int64)
        if seq_d1.dim() != 3 or seq_d1.shape != seq_d2.shape:
            raise ValueError("recommend_all: seq_d1 and seq_d2 must be [n, B, T] tensors of one shape")
        n, B, T = seq_d1.shape
        dom = torch.as_tensor(users["domain_id"]).to(dev, torch.int64).reshape(n, B)
        self._check_comp_batch(B)
        if not 1 <= int(k) <= 256:
            raise ValueError(f"k must be in 1..256, got {k}")
        pools = self._candidate_pools(pool)
        if min(int(q.numel()) for q in pools) < 1:
            raise ValueError("recommend_all: an empty candidate pool")
        pl = eng.plan(B, T, 2, need_grad=False)              # recommend()'s plan: the positive's slot and one negative, both zero
        zero = torch.zeros(n, B, dtype=torch.int64, device=dev)
        eng.stream.wait_stream(torch.cuda.current_stream())
        packed = eng.pack_epoch(pl, zero, zero.view(n, B, 1), seq_d1, seq_d2, torch.zeros(B, 2, device=dev), dom)
        eng.stream.wait_stream(torch.cuda.current_stream())
        ids, scores = eng.topk_epoch(pl, packed, pools, int(k), bool(exclude_history), use_graph=use_graph)
        torch.cuda.current_stream().wait_stream(eng.stream)
        eng.check_index_error(pl)
        return ids, scores

    # ---- the encode / score split and neighbours over the embedding spaces (csrc/neighbors.hip)
    @torch.no_grad()
    def encode_users(self, users: Dict[str, torch.Tensor], use_graph: bool = True) -> torch.Tensor:
        """The vectors recommend_all scores, taken out: users as recommend_all takes them; returns [n, B, D] float32 on the device, row
        (i, b) the own-domain vector of that row (for an isItC model the mixed vector) -- recommend_from_vectors on it gives
        recommend_all's rows bit for bit.  One graph replay a batch (SasrecEngine.encode_epoch; use_graph=False: the same launches,
        eagerly)."""
        eng = self.engine
        dev = eng.device
        seq_d1 = torch.as_tensor(users["seq_d1"]).to(dev, torch.int64)
        seq_d2 = torch.as_tensor(users["seq_d2"]).to(dev, torch.int64)
        if seq_d1.dim() != 3 or seq_d1.shape != seq_d2.shape:
            raise ValueError("encode_users: seq_d1 and seq_d2 must be [n, B, T] tensors of one shape")
        n, B, T = seq_d1.shape
        dom = torch.as_tensor(users["domain_id"]).to(dev, torch.int64).reshape(n, B)
        self._check_comp_batch(B)
        pl = eng.plan(B, T, 2, need_grad=False)              # recommend()'s plan
        zero = torch.zeros(n, B, dtype=torch.int64, device=dev)
        eng.stream.wait_stream(torch.cuda.current_stream())
        packed = eng.pack_epoch(pl, zero, zero.view(n, B, 1), seq_d1, seq_d2, torch.zeros(B, 2, device=dev), dom)
        eng.stream.wait_stream(torch.cuda.current_stream())
        raw = eng.encode_epoch(pl, packed, use_graph=use_graph)
        torch.cuda.current_stream().wait_stream(eng.stream)
        eng.check_index_error(pl)
        if raw.shape[1] == 1:
            return raw[:, 0]
        idx = (dom != 0).to(torch.int64).view(n, 1, B, 1).expand(n, 1, B, raw.shape[3])
        return torch.gather(raw, 1, idx)[:, 0].contiguous()

    @torch.no_grad()
    def recommend_from_vectors(self, u, domain_id, k: int = 10, pool=None, history=None):
        """The scorer alone: the k items the model scores highest for each stored user vector u [B, D] (encode_users' rows; any B -- the
        vectors are already mixed), in the domain domain_id [B], best first, ties to the lower id.  pool / k as in recommend();
        history [B, T] (optional): item ids to leave out of each row's list.  Returns (ids [B, k] int64, scores [B, k] float32) on the
        device, padded with -1 / -inf."""
        eng = self.engine
        dev = eng.device
        u = torch.as_tensor(u).to(dev, torch.float32).contiguous()
        if u.dim() != 2 or u.shape[1] != eng.D or u.shape[0] < 1:
            raise ValueError(f"recommend_from_vectors: u must be [B, {eng.D}] vectors")
        B = u.shape[0]
        dom = torch.as_tensor(domain_id).to(dev, torch.int64).reshape(B).contiguous()
        if not 1 <= int(k) <= 256:
            raise ValueError(f"k must be in 1..256, got {k}")
        if history is not None:
            history = torch.as_tensor(history).to(dev, torch.int64).contiguous()
            if history.dim() != 2 or history.shape[0] != B:
                raise ValueError("recommend_from_vectors: history must be [B, T] item ids")
        if eng.table_m is not None:
            eng.flush_table()
        pools = self._candidate_pools(pool)
        if min(int(q.numel()) for q in pools) < 1:
            raise ValueError("recommend_from_vectors: an empty candidate pool")
        ids = torch.empty(B, int(k), dtype=torch.int64, device=dev)
        scores = torch.empty(B, int(k), dtype=torch.float32, device=dev)
        flags = eng.flags_holder()
        eng.stream.wait_stream(torch.cuda.current_stream())
        eng.enqueue_topk_vectors(u, dom, pools, history, int(k), ids, scores, flags.err)
        torch.cuda.current_stream().wait_stream(eng.stream)
        eng.check_index_error(flags)
        return ids, scores

    NEIGHBOR_CHUNK = 4096         # queries per launch of similar_items

    @torch.no_grad()
    def neighbors(self, queries, base=None, k: int = 10, metric: str = "cosine", pool=None, exclude_self: bool = True):
        """Exact k nearest neighbours in an embedding space: queries -- int64 ids [Q] (rows of base) or float32 vectors [Q, D] -- against
        the rows of base, by "cosine" or "dot", best first, ties to the lower id.  base=None: the item table (pending lazy-Adam rows are
        flushed first); otherwise any contiguous float32 device tensor [N, D], D 64 / 128 -- stored encode_users output, say.  pool: the
        candidate rows (None: every row).  exclude_self (id queries only; ignored for vectors) leaves a query's own row out of its list.
        Returns (ids [Q, k] int64, scores [Q, k] float32) on the device, padded with -1 / -inf.  A score depends on its two rows only:
        bit-identical rows tie exactly."""
        eng = self.engine
        dev = eng.device
        if metric not in eng.NEIGHBOR_METRICS:
            raise ValueError(f"metric must be one of {sorted(eng.NEIGHBOR_METRICS)}, got {metric!r}")
        if not 1 <= int(k) <= 256:
            raise ValueError(f"k must be in 1..256, got {k}")
        if base is None:
            if eng.table_m is not None:
                eng.flush_table()
            base = eng.table
        if not (isinstance(base, torch.Tensor) and base.device == dev and base.dtype == torch.float32 and base.dim() == 2
                and base.is_contiguous() and base.shape[0] >= 1):
            raise ValueError("neighbors: base must be a contiguous float32 [N, D] tensor on the model's device")
        if base.shape[1] not in (64, 128):
            raise ValueError(f"neighbors: D must be 64 or 128, got {base.shape[1]}")
        q = torch.as_tensor(queries)
        if q.dtype.is_floating_point:
            q = q.to(dev, torch.float32).contiguous()
            if q.dim() != 2 or q.shape[1] != base.shape[1]:
                raise ValueError(f"neighbors: vector queries must be [Q, {base.shape[1]}]")
            exclude_self = False
        else:
            q = q.to(dev, torch.int64).reshape(-1).contiguous()
        if q.shape[0] < 1:
            raise ValueError("neighbors: no queries")
        if pool is not None:
            pool = self._candidate_pools(pool)[0]
            if pool.numel() < 1:
                raise ValueError("neighbors: an empty candidate pool")
        ids = torch.empty(q.shape[0], int(k), dtype=torch.int64, device=dev)
        scores = torch.empty(q.shape[0], int(k), dtype=torch.float32, device=dev)
        flags = eng.flags_holder()
        eng.stream.wait_stream(torch.cuda.current_stream())
        for c0 in range(0, q.shape[0], self.NEIGHBOR_CHUNK):      # chunked on the host: a whole pool can be the queries
            c1 = min(q.shape[0], c0 + self.NEIGHBOR_CHUNK)
            eng.enqueue_neighbors(q[c0:c1], base, pool, metric, int(k), bool(exclude_self), ids[c0:c1], scores[c0:c1], flags.err)
        torch.cuda.current_stream().wait_stream(eng.stream)
        eng.check_index_error(flags)
        return ids, scores

    def similar_items(self, ids, k: int = 10, metric: str = "cosine", pool=None):
        """The k items nearest to each item of `ids` in the trained item table, the item itself left out: neighbors(ids, base=None,
        exclude_self=True)."""
        return self.neighbors(ids, base=None, k=k, metric=metric, pool=pool, exclude_self=True)

    @torch.no_grad()
    def recommend_users(self, items, item_domain, vectors, vector_domain, k: int = 10, holders=None):
        """The audience of each item: the k rows of vectors [N, D] (stored encode_users output: contiguous float32 on the model's device,
        already mixed for an isItC model) that predictModule scores highest for table row items[q], among the rows whose
        vector_domain [N] equals item_domain[q], best first, ties to the lower row.  holders = (indices, offsets [Q + 1]): rows to leave
        out of each query's audience, indices[offsets[q] : offsets[q + 1]] for query q -- in any order, duplicates allowed; entries of the
        other domain or outside 0 .. N - 1 are ignored.  Returns (rows [Q, k] int64, scores [Q, k] float32) on the device, padded with
        -1 / -inf where fewer than k candidates exist.  A score equals recommend_from_vectors' for the same vector and item bit for bit.
        The user halves are formed once per call (SasrecEngine.enqueue_audience_halves); the queries go in chunks of
        engine.AUDIENCE_CHUNK."""
        eng = self.engine
        dev = eng.device
        if not (isinstance(vectors, torch.Tensor) and vectors.device == dev and vectors.dtype == torch.float32 and vectors.dim() == 2
                and vectors.is_contiguous() and vectors.shape[0] >= 1 and vectors.shape[1] == eng.D):
            raise ValueError(f"recommend_users: vectors must be a contiguous float32 [N, {eng.D}] tensor on the model's device")
        N = vectors.shape[0]
        if N >= 2 ** 31 - 1:
            raise ValueError(f"recommend_users: at most 2^31 - 2 vectors, got {N}")
        vdom = torch.as_tensor(vector_domain).to(dev, torch.int64).reshape(-1)
        if vdom.numel() != N:
            raise ValueError(f"recommend_users: vector_domain must have one entry per vector ({N}), got {vdom.numel()}")
        q = torch.as_tensor(items).to(dev, torch.int64).reshape(-1).contiguous()
        Q = q.shape[0]
        if Q < 1:
            raise ValueError("recommend_users: no query items")
        qdom = torch.as_tensor(item_domain).to(dev, torch.int64).reshape(-1).contiguous()
        if qdom.numel() != Q:
            raise ValueError(f"recommend_users: item_domain must have one entry per item ({Q}), got {qdom.numel()}")
        if not 1 <= int(k) <= 256:
            raise ValueError(f"k must be in 1..256, got {k}")
        hold = None
        if holders is not None:
            if not (isinstance(holders, (tuple, list)) and len(holders) == 2):
                raise ValueError("recommend_users: holders is None or a pair (indices, offsets [Q + 1])")
            h_idx = torch.as_tensor(holders[0]).to(dev, torch.int64).reshape(-1)
            h_off = torch.as_tensor(holders[1]).to(dev, torch.int64).reshape(-1).contiguous()
            if h_off.numel() != Q + 1:
                raise ValueError(f"recommend_users: holders' offsets must have Q + 1 = {Q + 1} entries, got {h_off.numel()}")
            if int(h_off[0]) != 0 or int(h_off[-1]) != h_idx.numel() or bool((h_off[1:] < h_off[:-1]).any()):
                raise ValueError("recommend_users: holders' offsets must rise from 0 to the number of indices")
            # ascending within each query's list: one sort of (query, row); rows outside 0 .. N - 1 become N, which no list holds
            seg = torch.repeat_interleave(torch.arange(Q, device=dev), h_off[1:] - h_off[:-1])
            idx = torch.where((h_idx < 0) | (h_idx >= N), torch.full_like(h_idx, N), h_idx)
            key = torch.sort(seg * (N + 1) + idx).values
            hold = ((key % (N + 1)).to(torch.int32).contiguous(), h_off)
        if eng.table_m is not None:
            eng.flush_table()
        isd1 = vdom != 0
        slots = (torch.nonzero(~isd1).reshape(-1).to(torch.int32).contiguous(), torch.nonzero(isd1).reshape(-1).to(torch.int32).contiguous())
        rows = torch.empty(Q, int(k), dtype=torch.int64, device=dev)
        scores = torch.empty(Q, int(k), dtype=torch.float32, device=dev)
        flags = eng.flags_holder()
        eng.stream.wait_stream(torch.cuda.current_stream())
        eng.enqueue_audience_halves(vectors, slots)
        for c0 in range(0, Q, eng.AUDIENCE_CHUNK):               # chunked on the host: a whole catalog can be the queries
            c1 = min(Q, c0 + eng.AUDIENCE_CHUNK)
            eng.enqueue_audience_topk(q[c0:c1], qdom[c0:c1], slots, None if hold is None else (hold[0], hold[1][c0:c1 + 1]), int(k),
                                      rows[c0:c1], scores[c0:c1], flags.err)
        torch.cuda.current_stream().wait_stream(eng.stream)
        eng.check_index_error(flags)
        return rows, scores

    RANK_LISTS_ROWS = 65536           # rows per amid_rank_lists_f32 call at most (the workspace holds a partial list per row and more)
    RANK_LISTS_CANDS = 1 << 26        # candidates per call at most, unless one row alone holds more

    def _candidate_lists(self, candidates, B: int, who: str):
        """`candidates` as (items int64 [n] on the device, offsets int64 [B + 1] on the device, the offsets on the host): a pair
        (items [n], offsets [B + 1]) -- validated on the host as recommend_users validates holders -- or a [B, C] tensor."""
        dev = self.engine.device
        if isinstance(candidates, (tuple, list)):
            if len(candidates) != 2:
                raise ValueError(f"{who}: candidates is a pair (items [n], offsets [B + 1]) or a [B, C] tensor")
            items = torch.as_tensor(candidates[0]).to(dev, torch.int64).reshape(-1).contiguous()
            off = torch.as_tensor(candidates[1]).to(torch.int64).reshape(-1)
            if off.numel() != B + 1:
                raise ValueError(f"{who}: the candidates' offsets must have B + 1 = {B + 1} entries, got {off.numel()}")
            off_h = off.cpu()
            if int(off_h[0]) != 0 or int(off_h[-1]) != items.numel() or bool((off_h[1:] < off_h[:-1]).any()):
                raise ValueError(f"{who}: the candidates' offsets must rise from 0 to the number of items")
            return items, off.to(dev).contiguous(), off_h
        c = torch.as_tensor(candidates)
        if c.dim() != 2 or c.shape[0] != B:
            raise ValueError(f"{who}: candidates is a pair (items [n], offsets [B + 1]) or a [B, C] tensor with B = {B} rows")
        off_h = torch.arange(B + 1, dtype=torch.int64) * c.shape[1]
        return c.to(dev, torch.int64).reshape(-1).contiguous(), off_h.to(dev), off_h

    def _rank_lists(self, u, u_dom_stride: int, dom, items, off, off_h, k, own, want_scores: bool, flags) -> "RankedLists":
        """The calls of one ranking on the engine's stream: rows in chunks of at most RANK_LISTS_ROWS rows and RANK_LISTS_CANDS
        candidates (cut on the host from the host's offsets; a row's result depends on its own list only, so not on the cut)."""
        eng = self.engine
        dev, B, D, n = eng.device, dom.shape[0], eng.D, int(items.numel())
        ids = scores = pos = ls = None
        if k is not None:
            ids = torch.empty(B, k, dtype=torch.int64, device=dev)
            scores = torch.empty(B, k, dtype=torch.float32, device=dev)
            pos = torch.empty(B, k, dtype=torch.int64, device=dev)
        if want_scores:
            ls = torch.empty(n, dtype=torch.float32, device=dev)
        uf = u.reshape(-1)
        c0 = 0
        while c0 < B:
            c1 = min(B, c0 + self.RANK_LISTS_ROWS)
            o0 = int(off_h[c0])
            while c1 > c0 + 1 and int(off_h[c1]) - o0 > self.RANK_LISTS_CANDS:
                c1 = c0 + max(1, (c1 - c0) // 2)
            o1 = int(off_h[c1])
            if o1 - o0 >= 2 ** 31 - 1:
                raise ValueError("rank lists: a list holds at most 2^31 - 2 candidates")
            if k is None and o1 == o0:                       # (scores only, and no candidate in these rows: nothing to write)
                c0 = c1
                continue
            sl = (lambda t: None if t is None else t[c0:c1])
            if c0 == 0 and c1 == B:
                off_c = off
            else:
                with torch.cuda.stream(eng.stream):          # (the chunk's offsets count from its first candidate)
                    off_c = off[c0:c1 + 1] - o0
            eng.enqueue_rank_lists(uf[c0 * D:], u_dom_stride, dom[c0:c1], items[o0:o1], off_c, o1 - o0,
                                   None if own is None else own[0], None if own is None else own[1], None if own is None else own[2][c0:c1],
                                   k, None if ls is None else ls[o0:o1], sl(ids), sl(scores), sl(pos), flags.err)
            c0 = c1
        return RankedLists(ids, scores, pos, ls)

    @staticmethod
    def _check_rank_k(k, list_scores: bool, who: str):
        if k is None:
            if not list_scores:
                raise ValueError(f"{who}: k=None asks for the lists' scores only, so list_scores must be true")
            return None
        if not 1 <= int(k) <= 256:
            raise ValueError(f"k must be in 1..256 or None, got {k}")
        return int(k)

    @torch.no_grad()
    def rank_candidates_from_vectors(self, u, domain_id, candidates, k=10, history=None, list_scores: bool = False) -> "RankedLists":
        """The scorer alone over each row's OWN candidate list: stored user vectors u [B, D] (encode_users' rows; any B), the domain
        domain_id [B], and candidates -- a pair (items int64 [n], offsets int64 [B + 1]): row b's list is items[offsets[b] :
        offsets[b + 1]], possibly empty, duplicates allowed -- or a [B, C] tensor of C candidates a row.  Returns
        RankedLists(ids, scores, positions, list_scores) of device tensors: the k best entries of each list ([B, k]; larger score
        first, ties to the lower id, further ties to the lower position; positions: the entry's index inside its own list; padded
        with -1 / -inf / -1), minus the ids of history [B, T] when given; and with list_scores=True every entry's score ([n], whatever
        history says).  k=None: the scores only.  A field not asked for is None.  A score equals recommend_from_vectors' for the same
        vector and item bit for bit (csrc/rank_lists.hip)."""
        eng = self.engine
        dev = eng.device
        who = "rank_candidates_from_vectors"
        u = torch.as_tensor(u).to(dev, torch.float32).contiguous()
        if u.dim() != 2 or u.shape[1] != eng.D or u.shape[0] < 1:
            raise ValueError(f"{who}: u must be [B, {eng.D}] vectors")
        B = u.shape[0]
        dom = torch.as_tensor(domain_id).to(dev, torch.int64).reshape(B).contiguous()
        k = self._check_rank_k(k, list_scores, who)
        items, off, off_h = self._candidate_lists(candidates, B, who)
        if history is not None:
            history = torch.as_tensor(history).to(dev, torch.int64).contiguous()
            if history.dim() != 2 or history.shape[0] != B:
                raise ValueError(f"{who}: history must be [B, T] item ids")
        if eng.table_m is not None:
            eng.flush_table()
        flags = eng.flags_holder()
        eng.stream.wait_stream(torch.cuda.current_stream())
        own = None if history is None or k is None else eng.enqueue_own_sets(history, history, dom)
        out = self._rank_lists(u, 0, dom, items, off, off_h, k, own, bool(list_scores), flags)
        torch.cuda.current_stream().wait_stream(eng.stream)
        eng.check_index_error(flags)
        return out

    @torch.no_grad()
    def rank_candidates(self, seq_d1, seq_d2, domain_id, candidates, k=10, exclude_history: bool = False,
                        list_scores: bool = False) -> "RankedLists":
        """rank_candidates_from_vectors for rows given as sequences (seq_d1 / seq_d2 [B, T], domain_id [B]): the rows are encoded as
        recommend() encodes them (comp models need exactly bs rows), so the result equals encode_users followed by
        rank_candidates_from_vectors bit for bit.  exclude_history leaves the ids of the row's own-domain sequence out of the top-K
        (off by default: the list is the caller's)."""
        eng = self.engine
        dev = eng.device
        who = "rank_candidates"
        seq_d1 = torch.as_tensor(seq_d1).to(dev, torch.int64).contiguous()
        seq_d2 = torch.as_tensor(seq_d2).to(dev, torch.int64).contiguous()
        if seq_d1.dim() != 2 or seq_d1.shape != seq_d2.shape:
            raise ValueError(f"{who}: seq_d1 and seq_d2 must be [B, T] tensors of one shape")
        B, T = seq_d1.shape
        dom = torch.as_tensor(domain_id).to(dev, torch.int64).reshape(B).contiguous()
        self._check_comp_batch(B)
        k = self._check_rank_k(k, list_scores, who)
        items, off, off_h = self._candidate_lists(candidates, B, who)
        if eng.table_m is not None:
            eng.flush_table()
        zero = torch.zeros(B, dtype=torch.int64, device=dev)
        label = torch.zeros(B, 2, device=dev)
        pl = eng.plan(B, T, 2, need_grad=False)              # recommend()'s plan
        eng.stream.wait_stream(torch.cuda.current_stream())
        eng.load_batch(pl, zero, zero.view(B, 1), seq_d1, seq_d2, label, dom)
        u, stride = eng.enqueue_user_vectors(pl)
        own = eng.enqueue_own_sets(seq_d1, seq_d2, dom) if exclude_history and k is not None else None
        out = self._rank_lists(u, stride, dom, items, off, off_h, k, own, bool(list_scores), pl)
        torch.cuda.current_stream().wait_stream(eng.stream)
        eng.check_index_error(pl)
        return out

    DIVERSIFY_ROWS = 65536            # rows per amid_mmr_lists_f32 call at most (the workspace holds a partial shortlist per row and more)
    DIVERSIFY_CANDS = 1 << 26         # entries per call at most, unless one row alone holds more

    @staticmethod
    def _check_diversify(k, lam, shortlist, who: str):
        if not 1 <= int(k) <= 256:
            raise ValueError(f"k must be in 1..256, got {k}")
        lam = float(lam)
        if not 0.0 <= lam <= 1.0:                            # (false for a NaN)
            raise ValueError(f"{who}: lam must be in [0, 1], got {lam}")
        shortlist = min(256, max(int(k), 100)) if shortlist is None else int(shortlist)
        if not int(k) <= shortlist <= 256:
            raise ValueError(f"{who}: shortlist must be in k..256, got {shortlist} with k {k}")
        return int(k), lam, shortlist

    @torch.no_grad()
    def diversify(self, candidates, relevance, k: int = 10, lam: float = 0.7, metric: str = "cosine", shortlist=None) -> "DiverseLists":
        """Greedy Maximal Marginal Relevance over each row's OWN list (csrc/diversify.hip): candidates as rank_candidates_from_vectors
        takes them -- a pair (items int64 [n], offsets int64 [B + 1]) or a [B, C] tensor --, relevance float32 [n] or [B, C], one per
        entry (rank_candidates' list_scores fit: an entry with a NaN relevance is absent).  The `shortlist` entries of a list with the
        largest relevance (ties to the lower id, then the lower position; None: min(256, max(k, 100))) are re-ranked: pick 1 is the
        head; every later pick is the entry with the largest lam * relevance - (1 - lam) * max_sim, max_sim = its largest similarity
        ("cosine" or "dot" over the item table: neighbors()' score, bit for bit) to the entries picked so far, among those whose id
        is not picked yet; ties to the lower id, then the lower position.  Returns DiverseLists(ids, scores, values, max_sims,
        positions) of [B, k] device tensors in pick order: scores = the picks' relevance, values / max_sims = the criterion and
        max_sim at the pick (pick 1: lam * relevance and 0), positions = the index inside the row's list; padded with -1 / -inf / -inf /
        -inf / -1.  lam = 1 gives the relevance order with ids deduplicated.  An id outside the table raises IndexError."""
        eng = self.engine
        dev = eng.device
        who = "diversify"
        if metric not in eng.NEIGHBOR_METRICS:
            raise ValueError(f"metric must be one of {sorted(eng.NEIGHBOR_METRICS)}, got {metric!r}")
        k, lam, shortlist = self._check_diversify(k, lam, shortlist, who)
        if isinstance(candidates, (tuple, list)):
            if len(candidates) != 2:
                raise ValueError(f"{who}: candidates is a pair (items [n], offsets [B + 1]) or a [B, C] tensor")
            B = int(torch.as_tensor(candidates[1]).numel()) - 1
        else:
            B = int(torch.as_tensor(candidates).shape[0])
        if B < 1:
            raise ValueError(f"{who}: no rows")
        items, off, off_h = self._candidate_lists(candidates, B, who)
        n = int(items.numel())
        rel = torch.as_tensor(relevance).to(dev, torch.float32).reshape(-1).contiguous()
        if rel.numel() != n:
            raise ValueError(f"{who}: relevance must have one entry per candidate ({n}), got {rel.numel()}")
        if eng.table_m is not None:
            eng.flush_table()
        out = DiverseLists(torch.empty(B, k, dtype=torch.int64, device=dev), torch.empty(B, k, dtype=torch.float32, device=dev),
                           torch.empty(B, k, dtype=torch.float32, device=dev), torch.empty(B, k, dtype=torch.float32, device=dev),
                           torch.empty(B, k, dtype=torch.int64, device=dev))
        flags = eng.flags_holder()
        eng.stream.wait_stream(torch.cuda.current_stream())
        c0 = 0
        while c0 < B:        # chunked on the host from the host's offsets, as _rank_lists: a row's picks depend on its own list only
            c1 = min(B, c0 + self.DIVERSIFY_ROWS)
            o0 = int(off_h[c0])
            while c1 > c0 + 1 and int(off_h[c1]) - o0 > self.DIVERSIFY_CANDS:
                c1 = c0 + max(1, (c1 - c0) // 2)
            o1 = int(off_h[c1])
            if o1 - o0 >= 2 ** 31 - 1:
                raise ValueError(f"{who}: a list holds at most 2^31 - 2 candidates")
            if c0 == 0 and c1 == B:
                off_c = off
            else:
                with torch.cuda.stream(eng.stream):          # (the chunk's offsets count from its first candidate)
                    off_c = off[c0:c1 + 1] - o0
            eng.enqueue_mmr_lists(items[o0:o1], off_c, rel[o0:o1], o1 - o0, metric, lam, k, shortlist, *(t[c0:c1] for t in out), flags.err)
            c0 = c1
        torch.cuda.current_stream().wait_stream(eng.stream)
        eng.check_index_error(flags)
        return out

    @torch.no_grad()
    def recommend_diverse(self, seq_d1, seq_d2, domain_id, k: int = 10, lam: float = 0.7, metric: str = "cosine", shortlist=None, pool=None,
                          exclude_history: bool = False) -> "DiverseLists":
        """recommend(seq_d1, seq_d2, domain_id, k=shortlist, pool, exclude_history) followed by diversify(k, lam, metric, shortlist) over
        each row's shortlist: that composition, bit for bit (positions: the rank in recommend()'s list; a row whose pool gave fewer than
        `shortlist` items is diversified over what it has).  Comp models need exactly bs rows, as for recommend()."""
        k, lam, shortlist = self._check_diversify(k, lam, shortlist, "recommend_diverse")
        ids, scores = self.recommend(seq_d1, seq_d2, domain_id, k=shortlist, pool=pool, exclude_history=exclude_history)
        return self.diversify_ranked(ids, scores, k=k, lam=lam, metric=metric)

    def diversify_ranked(self, ids, scores, k: int = 10, lam: float = 0.7, metric: str = "cosine") -> "DiverseLists":
        """diversify() over top-K results as recommend() and recommend_all() return them (ids / scores [B, M], M <= 256, padded with
        -1 / -inf at the end of a row): every row's M entries are its shortlist, the padding is left out."""
        M = int(ids.shape[1])
        some = ids >= 0
        if bool(some.all()):
            return self.diversify(ids, scores, k=k, lam=lam, metric=metric, shortlist=M)
        off = torch.zeros(ids.shape[0] + 1, dtype=torch.int64, device=ids.device)
        off[1:] = torch.cumsum(some.sum(1), 0)
        return self.diversify((ids[some], off), scores[some], k=k, lam=lam, metric=metric, shortlist=M)

    def check_indices(self) -> None:
        """Raise IndexError if any batch since the last check carried an item id outside the table (nn.Embedding raises on the spot,
        model_seq.py:27-29; the fused step flags it on the device and keeps going with row 0).  One device -> host read: call it
        where the loop synchronises anyway (the loss log every 20 iterations, the end of an epoch)."""
        pl = getattr(self, "_last_plan", None) or getattr(self, "_pool_plan", None)
        if pl is not None:
            self.engine.check_index_error(pl)

    def end_epoch_pool(self) -> None:
        """Hand the device back to torch's stream after an epoch of pool_step()s (the pool stays installed for the next epoch's
        refill; train_step() on the same plan is refused while it is -- use drop_epoch_pool())."""
        torch.cuda.current_stream().wait_stream(self.engine.stream)
        self.check_indices()

    def drop_epoch_pool(self) -> None:
        """Remove the pool of the current (Adam state, objective)."""
        eng = self.engine
        eng.sync()
        if getattr(self, "_pool_plan", None) is not None:
            eng.set_input_pool(self._pool_plan, None)

    def flush(self) -> None:
        """Bring lazily-updated table rows up to date (call before eval / state_dict() / checkpoints)."""
        self.engine.flush_table()
        self.engine.sync()

    def state_dict(self, *args, **kwargs):
        self.flush()
        return super().state_dict(*args, **kwargs)

    # -- training state (save / resume) -----------------------------------------------------------
    TRAINING_STATE_FORMAT = 1

    def save_training_state(self, path, **extra) -> None:
        """Write what a run needs to go on bit for bit from here (SasrecEngine.training_state: parameters and every Adam state with
        its raw lazy table state, step counters and dropout seeds) and `extra` -- plain data and tensors, e.g. the epoch and the loaders'
        state_dict()s -- as torch.save({"format": 1, "engine": ..., "extra": extra}), every tensor on the CPU."""
        torch.save({"format": self.TRAINING_STATE_FORMAT, "engine": self.engine.training_state(), "extra": extra}, path)

    def load_training_state(self, path) -> dict:
        """Load a save_training_state() file (or the dict torch.load made of one) into this model, in place, and return its `extra`.
        The model must have the file's configuration (ValueError naming the first field that differs).  Refused while an epoch pool is
        installed: the pool's batches are picked by the step counter that the load replaces."""
        eng = self.engine
        pl = getattr(self, "_pool_plan", None)
        if pl is not None and eng.input_pool(pl) is not None:
            raise ValueError("an epoch pool is installed (begin_epoch_pool): call drop_epoch_pool() before load_training_state()")
        d = path if isinstance(path, dict) else torch.load(path, map_location="cpu", weights_only=True)
        if d.get("format") != self.TRAINING_STATE_FORMAT:
            raise ValueError(f"not a training state of format {self.TRAINING_STATE_FORMAT} (format {d.get('format')!r})")
        eng.load_training_state(d["engine"])
        return d.get("extra", {})


# ------------------------------------------------------------------------------------------------
class _GatherFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weight, idx):
        L = lib()
        flat = idx.reshape(-1).contiguous()
        out = torch.empty(flat.numel(), weight.shape[1], dtype=weight.dtype, device=weight.device)
        err = torch.zeros(1, dtype=torch.int32, device=weight.device)
        is64 = 1 if flat.dtype == torch.int64 else 0
        if not is64 and flat.dtype != torch.int32:
            raise TypeError("item ids must be int64 or int32")
        L.call("amid_gather_rows_f32", weight.data_ptr(), weight.shape[0], weight.shape[1], flat.data_ptr(), is64, flat.numel(),
               out.data_ptr(), err.data_ptr(), torch.cuda.current_stream().cuda_stream)
        if int(err.item()):
            raise IndexError("index out of range in embItemLayerEnhance")
        ctx.save_for_backward(flat)
        ctx.shape = weight.shape
        return out.reshape(*idx.shape, weight.shape[1])

    _sort_ws = {}          # (device, n) -> the zero-filled sort workspace of backward

    @staticmethod
    def backward(ctx, g):
        (flat,) = ctx.saved_tensors
        L, s = lib(), torch.cuda.current_stream().cuda_stream
        n, D = flat.numel(), ctx.shape[1]
        if D not in (64, 128, 256):
            raise NotImplementedError(f"embItemLayerEnhance backward: the segment-reduce kernel is built for emb_dim in (64, 128, 256), got {D}")
        dev = g.device
        idx32 = flat.to(torch.int32)
        rows = g.reshape(n, D).contiguous()
        # the sort's workspace starts with a fixed ~8.4 MB head that must be zero once and that every call leaves consistent: one
        # zero-filled workspace per (device, n) for the life of the process instead of an allocation + memset per backward
        ws = _GatherFunction._sort_ws.get((dev, n))
        if ws is None:
            ws = _GatherFunction._sort_ws[(dev, n)] = torch.zeros(L.value("amid_sort_unique_workspace_bytes", n), dtype=torch.uint8, device=dev)
        pos, uniq = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        seg, nu = torch.empty(n + 1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        sof = torch.empty(n, dtype=torch.int32, device=dev)
        L.call("amid_sort_unique_i32", idx32.data_ptr(), n, ctx.shape[0], ws.data_ptr(), pos.data_ptr(), uniq.data_ptr(), seg.data_ptr(),
               sof.data_ptr(), nu.data_ptr(), s)
        ws2 = torch.empty(L.value("amid_segreduce_workspace_bytes", n, D), dtype=torch.uint8, device=dev)
        ug = torch.empty(n, D, dtype=torch.float32, device=dev)
        L.call("amid_embgrad_segreduce_f32", rows.data_ptr(), pos.data_ptr(), seg.data_ptr(), sof.data_ptr(), n, D, ws2.data_ptr(),
               ug.data_ptr(), s)
        U = int(nu.item())
        dense = torch.zeros(ctx.shape, dtype=torch.float32, device=dev)
        dense.index_copy_(0, uniq[:U].long(), ug[:U])
        return dense, None


class embItemLayerEnhance(nn.Module):
    """model_seq.py:22-29: plain lookup, no padding_idx (the pad id is an ordinary trainable row)."""

    def __init__(self, item_length, emb_dim):
        super().__init__()
        lib()
        self.emb_item = nn.Module()
        self.emb_item.register_parameter("weight", nn.Parameter(torch.randn(item_length, emb_dim, device="cuda")))

    def forward(self, item_id):
        return _GatherFunction.apply(self.emb_item.weight, item_id)


class predictModule(nn.Module):
    """model_seq.py:32-54 (forward only through the HIP scorer; training goes through SASRec)."""

    def __init__(self, emb_dim, hid_dim):
        super().__init__()
        lib()
        self.fc = nn.Sequential(nn.Linear(emb_dim * 2, hid_dim), nn.ReLU(), nn.Linear(hid_dim, 1)).cuda()
        self.emb_dim, self.hid_dim = emb_dim, hid_dim

    @torch.no_grad()
    def forward(self, user_spf1, user_spf2, i_feat):
        L = lib()
        B, NI, D = i_feat.shape
        u = torch.stack((user_spf1, user_spf2)).contiguous().float()
        items = i_feat.contiguous().float()
        p1 = torch.empty(B, NI, device=u.device)
        p2 = torch.empty(B, NI, device=u.device)
        L.call("amid_scorer_fwd_f32", u.data_ptr(), items.data_ptr(), self.fc[0].weight.data_ptr(), self.fc[0].bias.data_ptr(),
               self.fc[2].weight.data_ptr(), self.fc[2].bias.data_ptr(), None, None, B, NI, D, self.hid_dim, p1.data_ptr(), p2.data_ptr(),
               None, None, None, torch.cuda.current_stream().cuda_stream)
        return p1.squeeze(), p2.squeeze()


class Log2feats(nn.Module):
    """model_seq.py:331-387 as a standalone module (eval / inference): LN -> causal MHA -> FFN, two blocks."""

    def __init__(self, user_length, user_emb_dim, item_length, item_emb_dim, seq_len, hid_dim):
        super().__init__()
        lib()
        self.D, self.T = user_emb_dim, seq_len
        # a private two-domain engine whose table is the identity of the rows handed to forward()
        self._eng: Optional[SasrecEngine] = None
        names = [(n[len("sac1."):], s) for n, s in __import__("amid_amd.engine", fromlist=["x"]).sasrec_dense_names(seq_len, user_emb_dim, hid_dim)
                 if n.startswith("sac1.")]
        for n, shp in names:
            init = torch.ones(shp) if ("layernorm" in n and n.endswith("weight")) else torch.randn(shp) * 0.05
            if "layernorm" in n and n.endswith("bias"):
                init = torch.zeros(shp)
            _register_tree(self, n, nn.Parameter(init.cuda()))

    @torch.no_grad()
    def forward(self, log_seqs):
        B, T, D = log_seqs.shape
        eng = SasrecEngine(B * T + 2, D, self.T, 8, device=str(log_seqs.device))
        sd: Dict[str, torch.Tensor] = {"item_emb_layer.emb_item.weight": torch.cat((log_seqs.reshape(B * T, D).float(),
                                                                                     torch.zeros(2, D, device=log_seqs.device)))}
        own = dict(self.named_parameters())
        for name in eng.dense.slots:
            if name.startswith("sac"):
                sd[name] = own[name.split(".", 1)[1]]
            else:
                sd[name] = torch.zeros(eng.dense.slots[name][1], device=log_seqs.device)
        eng.load_state_dict(sd)
        pl = eng.plan(B, T, 2, need_grad=False)
        seq = torch.arange(B * T, device=log_seqs.device).reshape(B, T)
        z = torch.zeros(B, dtype=torch.long, device=log_seqs.device)
        eng.stream.wait_stream(torch.cuda.current_stream())
        eng.load_batch(pl, z, z.reshape(B, 1), seq, seq)
        eng.enqueue_prepare(pl, sparse=False)
        eng.enqueue_forward(pl, train=False, with_loss=False)
        # last LayerNorm (model_seq.py:385) of the first domain's rows, row by row on the host side of the ABI
        x = pl.x[2][: B * T]
        out = torch.empty_like(x)
        lib().call("amid_layernorm_rows_f32", x.data_ptr(), own["last_layernorm.weight"].data_ptr(), own["last_layernorm.bias"].data_ptr(),
                   B * T, D, SASREC_LN_EPS, out.data_ptr(), eng.s)          # model_seq.py:385
        torch.cuda.current_stream().wait_stream(eng.stream)
        return out.reshape(B, T, D)


# ------------------------------------------------------------------------------------------------
# signature-parity shells (constructors build the reference's parameters; forward is not built yet)
class embUserLayerEnhance(nn.Module):
    def __init__(self, user_length, emb_dim):          # model_seq.py:9-20 (never instantiated by the reference's models)
        super().__init__()
        self.emb_user_share = nn.Embedding(user_length, emb_dim)
        self.transd1 = nn.Linear(emb_dim, emb_dim)
        self.transd2 = nn.Linear(emb_dim, emb_dim)

    def forward(self, user_id):
        _not_built("embUserLayerEnhance", "model_seq.py:9-20")


def getBinaryTensor(imgTensor, boundary):              # model_seq.py:445-448
    return torch.where(imgTensor > boundary, torch.ones_like(imgTensor), torch.zeros_like(imgTensor))


class _CompFunction(torch.autograd.Function):
    """The standalone comp modules on the kernels BERT4Rec's front-of-encoder form uses (csrc/innercomp.hip): the rows are packed
    as the [2, B, T, D] pair those kernels take (slot 0 = the rows that keep their place, slot 1 = the rows mixed into the token
    group; InnerComp: the same rows twice) and slot 0's half of every result is what the module returns."""

    @staticmethod
    def forward(ctx, cross, threshold, seq_a, seq_b, w_nn, b_nn, w_bs, b_bs):
        L, st = lib(), torch.cuda.current_stream().cuda_stream
        B, T, D = seq_a.shape
        dev = seq_a.device
        f = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)      # noqa: E731
        xg = torch.stack((seq_a.float(), seq_b.float())).contiguous()
        par = [t.detach().float().contiguous() for t in (w_nn, b_nn, w_bs, b_bs)]
        two = lambda t: ptr_array([t.data_ptr(), t.data_ptr()])                # noqa: E731
        s, gate, S, Z, sw, x0 = f(2, B), f(2, B), f(2, T, D), f(2, T, D), f(2), f(2, B, 2 * T, D)
        L.call("amid_bert_comp_score_f32", xg.data_ptr(), B, T, D, cross, s.data_ptr(), st)
        L.call("amid_bert_comp_fwd_f32", xg.data_ptr(), s.data_ptr(), two(par[0]), two(par[1]), two(par[2]), two(par[3]), float(threshold),
               cross, B, T, D, gate.data_ptr(), S.data_ptr(), Z.data_ptr(), sw.data_ptr(), x0.data_ptr(), st)
        ctx.save_for_backward(xg, gate, S, sw, *par[:3])
        ctx.cross = cross
        return x0[0]

    @staticmethod
    def backward(ctx, dout):
        xg, gate, S, sw, w_nn, b_nn, w_bs = ctx.saved_tensors
        L, st = lib(), torch.cuda.current_stream().cuda_stream
        _, B, T, D = xg.shape
        dev = xg.device
        f = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)      # noqa: E731
        two = lambda t: ptr_array([t.data_ptr(), t.data_ptr()])                # noqa: E731
        dx0 = torch.zeros(2, B, 2 * T, D, dtype=torch.float32, device=dev)
        dx0[0] = dout
        dZ, dS, rows, dxg = f(2, T, D), f(2, T, D), f(2, T, 2), f(2, B, T, D)
        dw_nn, db_nn, dw_bs, db_bs = f(2, D, D), f(2, D), f(2, 1, B), f(2, 1)
        per = lambda t: ptr_array([t[0].data_ptr(), t[1].data_ptr()])          # noqa: E731
        L.call("amid_bert_comp_bwd_f32", xg.data_ptr(), dx0.data_ptr(), gate.data_ptr(), S.data_ptr(), sw.data_ptr(), two(w_nn), two(b_nn),
               two(w_bs), ctx.cross, B, T, D, dZ.data_ptr(), dS.data_ptr(), rows.data_ptr(), per(dw_nn), per(db_nn), per(dw_bs), per(db_bs),
               dxg.data_ptr(), st)
        # slot 1 received no gradient, so module 1's shares are exact zeros: slot 0 / module 0 carry everything
        d_a = dxg[0]
        d_b = dxg[1] if ctx.cross else None
        return None, None, d_a, d_b, dw_nn[0], db_nn[0], dw_bs[0], db_bs[0]


def _comp_check(mod, seq):
    lib()
    if seq.dim() != 3 or not seq.is_cuda:
        raise ValueError("expected a [b, n, d] tensor on the GPU")
    if seq.shape[0] != mod.bs:
        raise ValueError(f"the batch must hold exactly bs = {mod.bs} rows (trans_bs is Linear(bs, 1) over the batch), got {seq.shape[0]}")


class InnerComp(nn.Module):
    def __init__(self, user_emb_dim, bs, threshold):   # model_seq.py:450-457
        super().__init__()
        self.bs, self.threshold = bs, threshold
        self.trans_nn = nn.Linear(user_emb_dim, user_emb_dim)
        self.trans_bs = nn.Linear(bs, 1)

    def forward(self, seq):                            # model_seq.py:459-472: [b, n, d] -> [b, 2n, d]
        _comp_check(self, seq)
        return _CompFunction.apply(0, self.threshold, seq, seq.detach(), self.trans_nn.weight, self.trans_nn.bias, self.trans_bs.weight,
                                   self.trans_bs.bias)


class InterComp(nn.Module):
    def __init__(self, user_emb_dim, bs, threshold):   # model_seq.py:474-481
        super().__init__()
        self.bs, self.threshold = bs, threshold
        self.trans_nn = nn.Linear(user_emb_dim, user_emb_dim)
        self.trans_bs = nn.Linear(bs, 1)

    def forward(self, seq_d1, seq_d2):                 # model_seq.py:483-497: information seq_d2 --> seq_d1, [b, 2n, d]
        _comp_check(self, seq_d1)
        _comp_check(self, seq_d2)
        if seq_d1.shape != seq_d2.shape:
            raise ValueError("seq_d1 and seq_d2 must have the same shape")
        return _CompFunction.apply(1, self.threshold, seq_d1, seq_d2, self.trans_nn.weight, self.trans_nn.bias, self.trans_bs.weight,
                                   self.trans_bs.bias)


class GRU4Rec(nn.Module):
    def __init__(self, user_length, user_emb_dim, item_length, item_emb_dim, seq_len, hid_dim, bs, isInC, isItC, threshold1, threshold2,
                 isDR=False):                          # model_seq.py:58
        super().__init__()
        raise NotImplementedError("GRU4Rec is built in amid_amd.model_gru (class GRU4Rec, csrc/gru.hip): this constructor in model_seq is a stub "
                                  "kept until its callers move over (model_seq.py:56-113; INTEGRATION.md section A)")


class BERT4Rec(SASRec):
    """model_seq.py:248-309 on the HIP engine (isDR either way; isInC or isItC -- the reference fails with both -- put the comp
    module in front of the encoders, which then see 2 * seq_len tokens, :283-294): two stacks of two TransformerBlocks whose
    hidden size 128 / 4 heads / FFN 512 / dropout 0.1 the reference hard-codes (:264-267), so emb dims must be 128; no
    positional embedding; ONE key mask from seq_d2 > 0 for both stacks (:288); plain mean over time, then predictModule.
    Same constructor, forward signature, state_dict keys (transform{1,2}.{0,1}.*) and train_step() as SASRec above."""

    ENGINE_CLS = Bert4recEngine
    COMP_IN_FRONT = True         # BERT4Rec applies InnerComp / InterComp BEFORE the encoders (2T tokens, :283-294)
