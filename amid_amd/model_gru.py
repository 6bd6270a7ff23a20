"""``GRU4Rec`` of the reference's ``model_seq.py`` (:56-113) on the HIP engine: the third ``--model`` of the command line.

  GRU4Rec(user_length, user_emb_dim, item_length, item_emb_dim, seq_len, hid_dim, bs, isInC, isItC, threshold1, threshold2, isDR=False)
      forward(u_node, i_node, neg_samples, seq_d1, seq_d2, long_tail_mask_d1, long_tail_mask_d2, isTrain=True) -> (logits_d1, logits_d2)

Same constructor and forward signatures and the same ``state_dict`` keys as the reference (``item_emb_layer.emb_item.weight``,
``gru{1,2}.weight_ih_l0 / weight_hh_l0 / bias_ih_l0 / bias_hh_l0``, ``predictModule.fc.{0,2}.{weight,bias}``), and everything ``SASRec`` and
``BERT4Rec`` of ``model_seq.py`` here offer: the autograd path, the fused ``train_step`` / epoch pools, ``eval_ranks``, ``full_ranks``,
``recommend``, ``recommend_all``, ``save_training_state`` / ``load_training_state``.  The recurrent encoder runs in csrc/gru.hip
(engine_gru.py); emb dims must be 128.

``GRU4Rec`` is the plain model and refuses the three flags (its tests pin that); ``GRU4RecAMID`` below, same signatures, accepts any
combination of isInC / isItC / isDR and is what the command lines construct when ``--model gru4rec`` comes with one of them.  ``GRU4Rec``
stays until its test moves over, as the ``model_seq.GRU4Rec`` stub did.

(``amid_amd.model_seq.GRU4Rec`` is still the old stub that raises: a script written against the reference's ``from model_seq import *``
takes ``GRU4Rec`` from this module until that stub is retired -- INTEGRATION.md section A.)"""
from __future__ import annotations

from .engine_gru import Gru4recEngine
from .model_seq import SASRec


class GRU4Rec(SASRec):
    """model_seq.py:56-113: one single-layer GRU per domain from h0 = 0 on the plain gathered rows (no positional table, no mask: the pad
    id's row is an ordinary trained row), the plain mean over all T outputs, then predictModule.  nn.GRU's dropout = 0.5 does nothing with
    one layer, so train() and eval() compute the same thing and the step draws no random numbers.  Parameters start as the reference's do:
    nn.Embedding N(0, 1), nn.GRU and nn.Linear U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)) with fan_in = the hidden size for the GRU."""

    ENGINE_CLS = Gru4recEngine

    def __init__(self, user_length, user_emb_dim, item_length, item_emb_dim, seq_len, hid_dim, bs, isInC, isItC, threshold1, threshold2,
                 isDR=False, **kw):
        for flag, on in (("isInC", isInC), ("isItC", isItC), ("isDR", isDR)):
            if on:
                raise ValueError(f"GRU4Rec({flag}=True): this class is the plain model; the isInC / isItC / isDR variants are model_gru.GRU4RecAMID")
        if kw.get("compute", "f32") != "f32":
            raise ValueError("GRU4Rec: compute must be 'f32' (the recurrence runs on the fp32 matrix instructions only)")
        super().__init__(user_length, user_emb_dim, item_length, item_emb_dim, seq_len, hid_dim, bs, False, False, threshold1, threshold2,
                         isDR=False, **kw)

    def train_step(self, *args, exchange=None, **kw):
        if exchange is not None and exchange.world > 1:
            raise NotImplementedError("GRU4Rec: data-parallel training (world > 1) is not built")
        return super().train_step(*args, exchange=exchange, **kw)

    def pool_step(self, use_graph: bool = True, exchange=None, **kw):
        if exchange is not None and exchange.world > 1:
            raise NotImplementedError("GRU4Rec: data-parallel training (world > 1) is not built")
        return super().pool_step(use_graph=use_graph, exchange=exchange, **kw)


class GRU4RecAMID(GRU4Rec):
    """model_seq.py:56-113 with the three switches of its constructor, any combination (engine_gru.py):
      isInC (:89-91)   InnerComp on the plain gathered rows in front of the GRUs, which then step through 2 * seq_len tokens; state_dict gains
                       inc_d{1,2}.trans_nn / trans_bs;
      isItC (:97-101)  InterComp on the GRU outputs; state_dict gains itc_d{1,2}.*;
      isDR (:106-110)  predict_ips / predict_gfunc on the same (u, items): forward returns six outputs, train_step / pool_step take
                       dr_objective and ob_label as SASRec's do.
    With isInC or isItC every batch must hold exactly `bs` rows (trans_bs is Linear(bs, 1) over the batch).  With the flags all off this is
    GRU4Rec: the same state_dict, the same launches, and checkpoints of either class load into the other.  The variants live in a class
    of their own because GRU4Rec's refusal of the flags is pinned by its tests; GRU4Rec stays until that pin moves over."""

    def __init__(self, user_length, user_emb_dim, item_length, item_emb_dim, seq_len, hid_dim, bs, isInC, isItC, threshold1, threshold2,
                 isDR=False, **kw):
        if kw.get("compute", "f32") != "f32":
            raise ValueError("GRU4Rec: compute must be 'f32' (the recurrence runs on the fp32 matrix instructions only)")
        SASRec.__init__(self, user_length, user_emb_dim, item_length, item_emb_dim, seq_len, hid_dim, bs, bool(isInC), bool(isItC), threshold1,
                        threshold2, isDR=bool(isDR), **kw)
