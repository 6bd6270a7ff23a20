"""Host-side driver of the SASRec training hot path on one MI355X.

Mirrors the loop body of the reference's ``train()`` (train_sr.py:190-217) for
``SASRec`` (model_seq.py:390-443): forward, masked BCE, backward, optimizer --
as one sequence of launches of the hand-written HIP kernels in
``libamid_hip.so`` on a single HIP stream, capturable into a hipGraph.
PyTorch only provides device memory and the stream.

Memory layout (all fp32, resident in HBM for the life of the engine):
  table / m / v      [n_rows, D]   item embedding + lazy-Adam moments; ``last`` [n_rows] int32
  dense              flat buffer holding every other parameter in state_dict order (16-B aligned
                     slots); grad / Adam m / Adam v mirror it, so dense Adam and the data-parallel
                     all-reduce are one call each
  plan workspace     activations saved for backward, gradient scratch, sort / segment-reduce
                     workspaces -- allocated once per (B, T, n_items) shape
"""
from __future__ import annotations

import ctypes
import types
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from ._lib import absent, lib, prefixed, ptr_array

from .engine_dp import DataParallelMixin, HipMergeBackend      # noqa: F401  (re-exported)
from .engine_graph import GraphMixin
from .engine_io import InputMixin
from .engine_topk import TopkMixin
from .plan import (DR_HEADS, SASREC_HEADS, SASREC_LN_EPS, SASREC_P_DROP, FlatParams, SasrecPlan, Shape,      # noqa: F401  (re-exported)
                   sasrec_dense_names)

# The twelve parameter families of an encoder layer: (parameter name in include/amid_hip.h, state_dict name behind "sac{d}.").  The first
# four feed the layer's q / k / v launch, the other eight its out-projection / feed-forward launch.  THE list: every table derives from it.
SASREC_FAMILIES = (("ln1_w", "attention_layernorms.{l}.weight"), ("ln1_b", "attention_layernorms.{l}.bias"),
                   ("w_in", "attention_layers.{l}.in_proj_weight"), ("b_in", "attention_layers.{l}.in_proj_bias"),
                   ("w_o", "attention_layers.{l}.out_proj.weight"), ("b_o", "attention_layers.{l}.out_proj.bias"),
                   ("ln2_w", "forward_layernorms.{l}.weight"), ("ln2_b", "forward_layernorms.{l}.bias"),
                   ("w1", "forward_layers.{l}.conv1.weight"), ("b1", "forward_layers.{l}.conv1.bias"),
                   ("w2", "forward_layers.{l}.conv2.weight"), ("b2", "forward_layers.{l}.conv2.bias"))
# optional blocks a launch is not given (explicit nulls under the header's names): the weight-image riders, the sort riders
NO_W16_RIDERS = absent(("w_src", "w16_dst", "w16t_dst"), n_w=0, w_planes=0)
NO_SORT_RIDERS = absent(("sort_plan",), sort_phase=0)
NO_PACK = absent(("out_ids", "dense_src", "dense_dst", "err_flag"), n_out=0, pad_id=0, dense_n=0)      # a gradient tail that packs no exchange chunk
NO_UNIQ = absent(("uniq_ids", "n_uniq"))
NO_POS_ROWS = absent(("live", "dpos0", "dpos1"), B=0, T=0)          # a gradient tail whose reduce table holds the position rows' partial sums
NO_SCORER_SUMS = absent(("hidg", "u", "items", "dW1", "db1", "dW2", "db2"), NI=0, hid=0)
NO_FUSED_FFN = absent(("tmq", "step_state") + tuple("f" + n for n in ("h", "r", "ln_w", "w1T", "w2T", "woT", "dpre2", "dpre1", "dr", "d_o", "ln_part")),
                      flayer=0, train=0, p_drop=0.0)          # (the q / k / v backward of layer 0: no feed-forward chain below it)
LOSSES = ("bce", "softmax", "bpr")        # a train step's objective; the index is amid_scorer_listwise_fwd_bwd_f32's `kind` (1, 2)
NO_NEXT_QKV = absent(prefixed("n", dict.fromkeys(("qn", "q", "k", "v", "ln_w", "ln_b", "w_in", "b_in"))))


class SasrecEngine(InputMixin, GraphMixin, DataParallelMixin, TopkMixin):
    """Parameters, optimizer state and launch sequences for SASRec (isInC = isItC = isDR = False)."""

    HEADS = SASREC_HEADS
    PLAN_CLS = SasrecPlan
    EMB_DIMS = (64, 128)
    # ---- path switches (class attributes so that tests and the A/B tools can force a path; production never touches them) -----------
    #   STRIP_KERNELS / BF16_STRIP   the encoder on the register-resident strip kernels (fp32 / compute = "bf16")          [here]
    #   SEQ_FORWARD, LIVE_FORWARD    the forward as ONE launch; over the live sequences only in a train step            [at _live_list]
    #   SEQ_BACKWARD                 the backward's data gradients as ONE launch ("auto": n_CU < B <= 2 n_CU)          [at _seq_backward]
    #   FUSED_HEAD                   head forward + backward as one launch                                              [at _enqueue_fwd_bwd]
    #   SORT_RIDERS                  the step's index sort as extra workgroups of five main-stream launches             [at enqueue_sort]
    #   COMPACT_LIVE, COMPACT_MIN_IDX  the sparse side on the live sequences' positions only, for long index lists      [at live_forward_ok]
    #   DENSE_EXCHANGE               how the dense gradient crosses the ranks (engine_dp.DataParallelMixin)
    SHORT_TILE_BUILDS = False    # (BERT4Rec's row-tile kernels also exist as *_rt3 / *_rt4 / *_rt5: 48- / 64- / 80-row tiles, csrc/Makefile)
    STRIP_KERNELS = True         # fp32: the layer's GEMM chains run as register-resident strip kernels (csrc/sasrec_strip.hip)
    BF16_STRIP = True            # compute = "bf16" on the strip path (the forward's products in bf16)
    # (No path switch is read from the environment: A/B tools and tests set these class attributes -- bench.py --set NAME=VALUE,
    # profiles/tools/*.py -- and diagnostic BUILDS of the library are selected with AMID_LIB_PATH, amid_amd/_lib.py.)
    SEQ_FWD_VARIANT = 0          # != 0: amid_sas_seq_fwd_variant (which build of the one-launch forward runs: diagnostics)
    SEQ_BWD_VARIANT = 0          # != 0: amid_sas_seq_bwd_variant

    def _dense_names(self) -> List[Tuple[str, Tuple[int, ...]]]:
        return sasrec_dense_names(self.Tpos, self.D, self.hid, self.itc_bs, self.dr, self.inc_bs)

    def _alloc_model_buffers(self) -> None:
        D = self.D
        # transposed copies of the 24 square projection weights
        self.wT = torch.zeros(2, 2, 6, D * D, dtype=torch.float32, device=self.device)     # [layer][domain][q,k,v,o,c1,c2]

    def __init__(self, item_length: int, emb_dim: int, seq_len: int, hid_dim: int, device="cuda:0", lr: float = 5e-4,
                 betas=(0.9, 0.999), eps: float = 1e-8, seed: int = 0, itc_bs: int = 0, itc_threshold: float = 0.5, dr: bool = False,
                 dr_e_w: float = 0.1, compute: str = "f32", inc_bs: int = 0, inc_threshold: float = 0.5, loss: str = "bce",
                 hard_negs: int = 0, hard_skip: int = 0):
        """itc_bs > 0: SASRec(isItC=True, bs=itc_bs, threshold2=itc_threshold) -- InterComp after the encoders
        (model_seq.py:426-431); every batch must then hold exactly itc_bs rows (trans_bs is Linear(bs, 1) over the batch).
        loss: the objective of a train step over a row's candidates (column 0 the positive): "bce" the reference's masked BCE
        (train_sr.py:203-212), "softmax" / "bpr" sampled softmax / BPR on the own domain's logits (csrc/head_listwise.hip; DESIGN.md
        section 17).  Evaluation (test(), eval_ranks, recommend*) does not depend on it.
        hard_negs = H > 0 (with loss "softmax" / "bpr"): of a row's sampled negatives only the H ranked hard_skip .. hard_skip + H - 1 by the
        current model's own-domain logit enter the objective and the backward (csrc/head_mined.hip); 0: all of them."""
        if loss not in LOSSES:
            raise ValueError(f"loss must be one of {LOSSES}, got {loss!r}")
        if loss != "bce":
            why = ("isDR: the doubly-robust objectives are written on the BCE value" if dr else
                   "compute = 'bf16': the listwise step is built in fp32" if compute == "bf16" else
                   "isInC / a comp module in front of the encoders: the listwise step is not built for it" if inc_bs else "")
            if why:
                raise ValueError(f"loss = {loss!r} is refused with {why}")
        self.loss = loss
        hard_negs, hard_skip = int(hard_negs), int(hard_skip)
        if hard_negs < 0 or hard_skip < 0:
            raise ValueError(f"hard_negs and hard_skip must be >= 0, got {hard_negs} and {hard_skip}")
        if hard_negs > 0 and loss == "bce":
            raise ValueError(f"hard_negs = {hard_negs} needs loss 'softmax' or 'bpr': the masked BCE has one negative a row, nothing to mine")
        if hard_skip > 0 and hard_negs == 0:
            raise ValueError(f"hard_skip = {hard_skip} without hard_negs: there is no mined list to skip the top of")
        self.hard_negs, self.hard_skip = hard_negs, hard_skip
        L = lib()        # raises AmidLibraryError when the HIP library is missing: no fallback
        if self.SEQ_FWD_VARIANT:          # A/B measurements of the fused forward's builds (amid_sas_seq_fwd_variant)
            L.value("amid_sas_seq_fwd_variant", int(self.SEQ_FWD_VARIANT))
        if self.SEQ_BWD_VARIANT:          # ... and of the fused backward's (amid_sas_seq_bwd_variant)
            L.value("amid_sas_seq_bwd_variant", int(self.SEQ_BWD_VARIANT))
        self.itc_bs, self.itc_threshold = int(itc_bs), float(itc_threshold)
        # inc_bs > 0: SASRec(isInC=True, bs=inc_bs, threshold1=inc_threshold) -- InnerComp on the gathered rows before the encoders,
        # which then see 2 * seq_len tokens per row (model_seq.py:398-401, :422-424; csrc/innercomp.hip); batches of exactly inc_bs rows
        self.inc_bs, self.inc_threshold = int(inc_bs), float(inc_threshold)
        # dr: SASRec(isDR=True) -- predict_ips / predict_gfunc heads and the two objectives of train_sr_dr.py; dr_mode selects
        # the objective of the next train step (0: loss_cls + dr_e_w * loss_dr_e, 1: loss_dr_r), see select_optimizer()
        self.dr, self.dr_e_w, self.dr_mode = bool(dr), float(dr_e_w), 0
        # compute = "bf16": the dense projections' matrix products take bf16 operands (fp32 accumulate, fp32 everything else);
        # BASELINE.json configs[2].  "f32" (default): exact fp32 products.
        if compute not in ("f32", "bf16"):
            raise ValueError(f"compute must be 'f32' or 'bf16', got {compute!r}")
        if compute == "bf16" and emb_dim != 128:
            raise ValueError("the bf16 matrix-core kernels are built for emb_dim 128")
        self.compute, self.mma_bf16 = compute, 1 if compute == "bf16" else 0
        if emb_dim not in self.EMB_DIMS:
            raise ValueError(f"amid_amd {type(self).__name__} kernels are built for emb_dim in {self.EMB_DIMS}, got {emb_dim}")
        self.device = torch.device(device)
        # every kernel of the engine runs on this (non-default, hence capturable) HIP stream
        self.stream = torch.cuda.Stream(device=self.device)
        # the index sort only feeds the segment reduce after backward: it runs on this side stream, beside the forward pass
        self.side = torch.cuda.Stream(device=self.device)
        self.ev_idx = torch.cuda.Event()
        self.ev_sorted = torch.cuda.Event()
        self.n_rows, self.D, self.T, self.hid, self.H = int(item_length), int(emb_dim), int(seq_len), int(hid_dim), self.HEADS
        self.Tpos = 2 * self.T if getattr(self, "inc_bs", 0) else self.T          # rows of the pos_emb tables
        D = self.D
        self.dense = FlatParams(self._dense_names(), self.device)
        self.table = torch.zeros(self.n_rows, D, dtype=torch.float32, device=self.device)
        self.table_m: Optional[torch.Tensor] = None        # allocated on the first optimizer use
        self.table_v: Optional[torch.Tensor] = None
        self.table_last: Optional[torch.Tensor] = None
        self._alloc_model_buffers()
        self.hyper = dict(lr=lr, beta1=betas[0], beta2=betas[1], eps=eps)
        self.seed = int(seed)
        self.step = 0
        self._st_bytes = L.value("amid_step_state_bytes")
        # empty, not zeros: a zero fill on torch's stream is unordered against the copy _push_step_state issues on the engine's stream and
        # could land after it (a step then ran with seed 0 and zero Adam coefficients: found by tests/test_gpu_fused_opt.py, round 6)
        self.step_state = torch.empty(self._st_bytes, dtype=torch.uint8, device=self.device)
        self._push_step_state()
        self.plans: Dict[Tuple[int, int, int, bool], SasrecPlan] = {}
        self.grad_scale = 1.0
        self.opt_bank, self._banks = 0, {}          # several Adam states over the same parameters (train_sr_dr.py:668-669)
        torch.cuda.synchronize(self.device)
        self._ptr_cache: Dict[str, object] = {}

    @property
    def s(self) -> int:
        return self.stream.cuda_stream

    def sync(self) -> None:
        self.join_sort()
        self.stream.synchronize()

    # ------------------------------------------------------------------ state
    def _push_step_state(self) -> None:
        L = lib()
        host = (ctypes.c_ubyte * self._st_bytes)()
        L.call("amid_step_state_pack", ctypes.addressof(host), self.seed, self.step, self.hyper["lr"], self.hyper["beta1"],
               self.hyper["beta2"], self.hyper["eps"])
        with torch.cuda.stream(self.stream):
            self.step_state.copy_(torch.frombuffer(bytearray(host), dtype=torch.uint8), non_blocking=False)

    @staticmethod
    def rank_seed(seed: int, rank: int) -> int:
        """Dropout seed of data-parallel rank `rank`: the counters are indexed by the LOCAL row, so ranks sharing one seed would apply
        the same masks to their different shards -- correlated noise a single-GPU run at the global batch does not have.  Weights
        are initialised from `seed` itself on every rank (identical replicas)."""
        return (int(seed) + 0x9E3779B97F4A7C15 * int(rank)) & 0x7FFFFFFFFFFFFFFF

    def set_step(self, step: int, seed: Optional[int] = None) -> None:
        self.step = int(step)
        if seed is not None:
            self.seed = int(seed)
        self._push_step_state()

    def set_lr(self, lr: float) -> None:
        self.hyper["lr"] = float(lr)
        self._push_step_state()

    def _ensure_opt_state(self) -> None:
        if self.table_m is None:
            self.table_m = torch.zeros_like(self.table)
            self.table_v = torch.zeros_like(self.table)
            self.table_last = torch.zeros(self.n_rows, dtype=torch.int32, device=self.device)
            # the zero fills run on torch's stream, the step that needs them on the engine's: without this a first step enqueued straight away
            # read moments and stamps that were not zero yet (a catch-up replaying garbage gaps: found by tests/test_gpu_fused_opt.py, round 6)
            torch.cuda.synchronize(self.device)

    def select_optimizer(self, k: int, lr: Optional[float] = None) -> None:
        """Switch to Adam state `k` (its own moments, step counter and learning rate over the SAME parameters): the reference's
        doubly-robust trainer alternates two torch.optim.Adam instances (train_sr_dr.py:668-669, :222-224, :396-398).  Pending
        lazy updates of the state being left are applied first (one pass over the table), so rows never owe moves to an idle state."""
        if k == self.opt_bank:
            if lr is not None and lr != self.hyper["lr"]:
                self.set_lr(lr)
            return
        self.flush_table()
        self.sync()
        fp = self.dense
        self._banks[self.opt_bank] = dict(m=fp.m, v=fp.v, tm=self.table_m, tv=self.table_v, tl=self.table_last, st=self.step_state,
                                          step=self.step, lr=self.hyper["lr"], seed=self.seed)
        b = self._banks.get(k)
        if b is None:
            b = dict(m=torch.zeros_like(fp.m), v=torch.zeros_like(fp.v), tm=None, tv=None, tl=None,
                     st=torch.empty(self._st_bytes, dtype=torch.uint8, device=self.device), step=0,
                     lr=self.hyper["lr"] if lr is None else float(lr), seed=self.seed + 0x9E3779B9 * k)
        fp.m, fp.v, self.table_m, self.table_v, self.table_last = b["m"], b["v"], b["tm"], b["tv"], b["tl"]
        self.step_state, self.step, self.seed = b["st"], b["step"], b["seed"]
        self.hyper["lr"] = b["lr"] if lr is None else float(lr)
        self.opt_bank = k
        self._push_step_state()
        torch.cuda.synchronize(self.device)

    def _graph_key(self) -> Tuple[int, int]:
        return (self.opt_bank, self.dr_mode if self.dr else 0)

    def plan(self, B: int, T: int, NI: int, need_grad: bool) -> SasrecPlan:
        key = (B, T, NI, need_grad)
        if key not in self.plans:
            inc = getattr(self, "inc_bs", 0)
            if (2 * T if inc else T) > self.Tpos:
                raise ValueError(f"sequence length {T} exceeds pos_emb size {self.Tpos}" + (" / 2 (isInC)" if inc else ""))
            self.plans[key] = self.PLAN_CLS(self, Shape(B, T, NI, 2 * T if inc else 0), need_grad)
            torch.cuda.synchronize(self.device)      # buffers were zero-filled on torch's stream
        return self.plans[key]

    # ------------------------------------------------------------------ pointer helpers
    def _pp(self, fmt: str, buf: Optional[torch.Tensor] = None, extra: int = 0):
        """Host array (domain 0, domain 1) of device pointers of a per-domain parameter."""
        return self._cached((fmt, 0 if buf is None else buf.data_ptr(), extra),
                            lambda: ptr_array([self.dense.ptr(fmt.format(d=d), buf, extra) for d in (1, 2)]))

    def _wT(self, layer: int, which: int):
        """Host array (domain 0, domain 1) of the transposed projection weight `which` (q, k, v, o, c1, c2) of `layer`: fp32 transposes,
        or -- pl.strip with compute = "bf16" -- their bf16 fragment images (amid_sas_weights_bf16, refreshed by enqueue_backward)."""
        bf = self._bf16_bwd
        p3 = self._p3_bwd
        return self._cached(("wT16x3" if p3 else "wT16" if bf else "wT", layer, which), lambda: ptr_array(
            [(self.wT16x3 if p3 else self.wT16 if bf else self.wT)[layer, g, which].data_ptr() for g in (0, 1)]))

    # ---- named pointer tables: parameter name of include/amid_hip.h -> value, bound by L.call_named.  Tables of parameters live on the
    # engine, tables of a plan's tensors on the plan; each is built once (the buffers never move: engine_graph restores in place).
    def _cached(self, key, build):
        c = self._ptr_cache.get(key)
        if c is None:
            c = self._ptr_cache[key] = build()
        return c

    def _fams(self):
        """The twelve parameter families [layer][domain] of the one-launch encoder entry points."""
        fp = self.dense
        return self._cached("fams", lambda: {n: ptr_array([fp.ptr(f"sac{d}." + fmt.format(l=l)) for l in (0, 1) for d in (1, 2)])
                                             for n, fmt in SASREC_FAMILIES})

    def _lay(self):
        """Per layer: the families as (domain 0, domain 1) pairs, what the strip and row-tile launches take."""
        return self._cached("lay", lambda: [{n: self._pp("sac{d}." + fmt.format(l=l)) for n, fmt in SASREC_FAMILIES} for l in (0, 1)])

    def _pos(self):
        fp = self.dense
        return self._cached("pos", lambda: dict(pos0=fp.ptr("sac1.pos_emb.weight"), pos1=fp.ptr("sac2.pos_emb.weight")))

    def _scorer(self, names=("w1", "b1", "w2", "b2"), grad: bool = False):
        """The scorer's four pointers (grad: their gradients') under `names`: the header spells them w1 .. b2, sw1 .. sb2 beside the
        encoder's own w1 .. b2, dW1 .. db2."""
        fp = self.dense
        return self._cached(("scorer", names, grad), lambda: dict(zip(names, (
            fp.ptr("predictModule.fc." + n, fp.grad if grad else None) for n in ("0.weight", "0.bias", "2.weight", "2.bias")))))

    def _last_ln(self, names=("ln_w", "ln_b")):
        """The last LayerNorm's (domain 0, domain 1) gains and biases under `names` (last_ln_w / last_ln_b in the head-on-forward entries)."""
        return self._cached(("last_ln", names), lambda: dict(zip(names, (self._pp("sac{d}.last_layernorm.weight"),
                                                                          self._pp("sac{d}.last_layernorm.bias")))))

    def _wT_fams(self, bf16: bool):
        """amid_sas_seq_bwd_f32's transposed-weight families [layer][domain]: the fp32 transposes or their one-plane bf16 images."""
        buf = self.wT16 if bf16 else self.wT
        return self._cached(("wT_fams", bool(bf16)), lambda: {
            n: ptr_array([buf[l, g, j].data_ptr() for l in (0, 1) for g in (0, 1)]) for j, n in enumerate(("wqT", "wkT", "wvT", "woT", "w1T", "w2T"))})

    def _wT_lists(self):
        """(src, dst, n) of a step's 24 fp32 weight transposes: in_proj's q / k / v blocks, out_proj, conv1, conv2 of both layers and domains."""
        def build():
            fp, D, src, dst = self.dense, self.D, [], []
            for l in (0, 1):
                for g in (0, 1):
                    pre = f"sac{g + 1}"
                    src += [fp.ptr(f"{pre}.attention_layers.{l}.in_proj_weight", None, j * D * D) for j in range(3)]
                    src += [fp.ptr(f"{pre}.attention_layers.{l}.out_proj.weight"), fp.ptr(f"{pre}.forward_layers.{l}.conv1.weight"),
                            fp.ptr(f"{pre}.forward_layers.{l}.conv2.weight")]
                    dst += [self.wT[l, g, w].data_ptr() for w in range(6)]
            return ptr_array(src), ptr_array(dst), len(src)
        return self._cached("wT_lists", build)

    @staticmethod
    def _seq_ptrs(pl: SasrecPlan):
        """The plan's per-layer tensors as host pointer arrays: the layers' inputs and what the one-launch forward saves for the backward."""
        if not hasattr(pl, "seq_ptrs"):
            pa = lambda ts: ptr_array([t.data_ptr() for t in ts])          # noqa: E731
            pl.seq_ptrs = dict(x_in=pa(pl.x[:2]), qn=pa(pl.qn), q=pa(pl.q), k=pa(pl.k), v=pa(pl.v), o=pa(pl.o), stats=pa(pl.stats), r=pa(pl.r),
                               y=pa(pl.y), h=pa(pl.h))
        return pl.seq_ptrs

    @staticmethod
    def _seq_grad_ptrs(pl: SasrecPlan):
        """... and what the one-launch backward writes."""
        if not hasattr(pl, "seq_grad_ptrs"):
            pa = lambda ts: ptr_array([t.data_ptr() for t in ts])          # noqa: E731
            pl.seq_grad_ptrs = dict(dpre2=pa(pl.dpre2), dpre1=pa(pl.dpre1), dr=pa(pl.dr), dq=pa(pl.dq_l), dk=pa(pl.dk_l), dv=pa(pl.dv_l),
                                    ln1_part=pa(pl.ln1_part_s), ln2_part=pa(pl.ln2_part_s))
        return pl.seq_grad_ptrs

    @staticmethod
    def _on_plan(pl: SasrecPlan, name: str, build):
        """A table of the plan's own tensors, built once (a plan's buffers never move)."""
        t = pl.__dict__.get(name)
        if t is None:
            t = pl.__dict__[name] = build()
        return t

    def _marshal(self, pl: SasrecPlan):
        """The index marshal's batch: the plan's static inputs, their packed image and the lists the packing launches write (T: the
        batch's own sequence length, not the encoders')."""
        shp, p = pl.shape, lambda n: getattr(pl, n).data_ptr()          # noqa: E731
        return self._on_plan(pl, "marshal_tab", lambda: dict(
            i_node=p("in_i_node"), neg=p("in_neg"), seq_d1=p("in_seq_d1"), seq_d2=p("in_seq_d2"), in_pack=p("in_pack"), in_words=pl.in_words,
            B=shp.B, T=shp.T, n_neg=shp.NI - 1, n_rows=self.n_rows, idx_all=p("idx_all"), idx_c=p("idx_c"), row_c=p("row_c"), live=p("live"),
            domain=p("domain"), err_flag=p("err")))

    def _seg(self, pl: SasrecPlan):
        """The segment reduce of the table-row gradients: the rows, the sorted positions and their runs, the workspace, the reduced rows."""
        return self._on_plan(pl, "seg_tab", lambda: dict(
            grad_rows=pl.dxg.data_ptr(), pos_sorted=pl.pos_sorted.data_ptr(), seg_off=pl.seg_off.data_ptr(), seg_of=pl.seg_of.data_ptr(),
            workspace=pl.seg_ws.data_ptr(), uniq_grad=pl.uniq_grad.data_ptr()))

    def _uniq(self, pl: SasrecPlan):
        """The step's unique rows: their ids and their count."""
        return self._on_plan(pl, "uniq_tab", lambda: dict(uniq_ids=pl.uniq_ids.data_ptr(), n_uniq=pl.n_uniq.data_ptr()))

    def _saved(self, pl: SasrecPlan, l: int):
        """What layer `l`'s forward saves for its backward, under the strip and row-tile entries' names (xo: the layer's output)."""
        return self._on_plan(pl, f"saved_tab{l}", lambda: dict(
            {n: getattr(pl, n)[l].data_ptr() for n in ("x", "qn", "q", "k", "v", "o", "stats", "r", "y", "h")}, xo=pl.x[l + 1].data_ptr()))

    def _qkv_block(self, pl: SasrecPlan, l: int, pre: str = ""):
        """Layer `l`'s LayerNorm + q / k / v under its own launch's names; pre = "n": as the next layer's block of the launch in front of it."""
        lay = self._lay()[l]
        return self._on_plan(pl, f"qkv_tab{l}{pre}", lambda: prefixed(pre, dict(
            {n: getattr(pl, n)[l].data_ptr() for n in ("qn", "q", "k", "v")}, ln_w=lay["ln1_w"], ln_b=lay["ln1_b"], w_in=lay["w_in"], b_in=lay["b_in"])))

    def _ffn_bwd_block(self, pl: SasrecPlan, l: int, rows: bool, fused: bool = False):
        """Layer l's feed-forward / out-projection backward under its own launch's names: what it reads, the transposes in the form this
        backward multiplies (_wT), what it writes.  rows: the row-tile kernels' partials over the live rows.  fused: under the names of the
        q / k / v backward of the layer above, which runs this chain in the same launch (fh, fr, fln_w ...)."""
        kind = f"{int(self._p3_bwd)}{int(self._bf16_bwd)}{int(bool(rows))}"
        if fused:
            return self._on_plan(pl, f"fused_ffn_bwd_tab{l}{kind}", lambda: prefixed("f", self._ffn_bwd_block(pl, l, rows)))
        return self._on_plan(pl, f"ffn_bwd_tab{l}{kind}", lambda: dict(
            self._grads(pl, l), h=pl.h[l].data_ptr(), r=pl.r[l].data_ptr(), ln_w=self._pp(f"sac{{d}}.forward_layernorms.{l}.weight"),
            w1T=self._wT(l, 4), w2T=self._wT(l, 5), woT=self._wT(l, 3), layer=l, d_o=pl.d_o.data_ptr(),
            ln_part=(pl.ln2_part_v if rows else pl.ln2_part)[l].data_ptr()))

    def _qkv_bwd_block(self, pl: SasrecPlan, l: int, rows: bool):
        """... and its q / k / v + LayerNorm1 backward."""
        kind = f"{int(self._p3_bwd)}{int(self._bf16_bwd)}{int(bool(rows))}"
        return self._on_plan(pl, f"qkv_bwd_tab{l}{kind}", lambda: dict(
            self._grads(pl, l), x=pl.x[l].data_ptr(), ln_w=self._pp(f"sac{{d}}.attention_layernorms.{l}.weight"), wqT=self._wT(l, 0),
            wkT=self._wT(l, 1), wvT=self._wT(l, 2), ln_part=(pl.ln1_part_v if rows else pl.ln1_part)[l].data_ptr()))

    def _grads(self, pl: SasrecPlan, l: int):
        """Layer `l`'s gradient outputs (d_o and the encoder-input gradient are shared by the layers: given by name)."""
        return self._on_plan(pl, f"grads_tab{l}", lambda: dict(
            dq=pl.dq_l[l].data_ptr(), dk=pl.dk_l[l].data_ptr(), dv=pl.dv_l[l].data_ptr(), dr=pl.dr[l].data_ptr(), dpre1=pl.dpre1[l].data_ptr(),
            dpre2=pl.dpre2[l].data_ptr()))

    # (the two Adam tables are read from the tensors at every launch, never cached: select_optimizer rebinds them, and a state dropped and
    # made again by load_training_state has new buffers under its old number)
    def _adam_dense(self, g: Optional[torch.Tensor] = None):
        """Dense Adam over the flat buffer with the current state's moments: p, m, v, g, n (g: the engine's own gradient buffer or a caller's)."""
        fp = self.dense
        return dict(p=fp.data.data_ptr(), m=fp.m.data_ptr(), v=fp.v.data_ptr(), g=(fp.grad if g is None else g).data_ptr(), n=fp.numel)

    def _adam_rows(self):
        """Lazy row Adam: the table, the current state's moments (m_tab, v_tab -- m, v are the dense ones) and the rows' step stamps."""
        return dict(table=self.table.data_ptr(), m_tab=self.table_m.data_ptr(), v_tab=self.table_v.data_ptr(), last=self.table_last.data_ptr())

    def _dpos(self):
        """The position rows' gradients."""
        fp = self.dense
        return self._cached("dpos", lambda: dict(dpos0=fp.ptr("sac1.pos_emb.weight", fp.grad), dpos1=fp.ptr("sac2.pos_emb.weight", fp.grad)))

    def _k1_head(self, pl: SasrecPlan, pos0, pos1, tmq, tr: int, p_drop: float, n_item_rows: int):
        """What every form of the gather K1 takes behind the table (the replay form takes the table with its Adam state: _adam_rows)."""
        shp = pl.shape
        return dict(idx_all=pl.idx_all.data_ptr(), pos0=pos0, pos1=pos1, B=shp.B, T=shp.Tenc, D=self.D, n_item_rows=n_item_rows,
                    xg=pl.xg.data_ptr(), tmq=tmq, step_state=self.step_state.data_ptr(), train=tr, p_drop=p_drop, stream=self.s)

    def _w16_riders(self, transposes: bool = True):
        """The weight images a launch's extra workgroups write: three bf16 planes of the 24 encoder weights (+ of their transposes)."""
        src, w16 = self._w16_images(3)
        return dict(w_src=src, n_w=24, w_planes=3, w16_dst=w16.data_ptr(), w16t_dst=self._wT16x3_buf().data_ptr() if transposes else None)

    _bf16_bwd = False          # set per backward: the strip backward's products take bf16 images (compute = "bf16" on the strip path)
    _p3_bwd = False            # set per backward: ... three-plane images (compute = "fp32", products on bf16 pieces)
    # compute = "fp32": the strip backward's data-gradient products on the bf16 matrix cores at fp32 accuracy (three bf16 pieces per operand,
    # six piece pairs: csrc/strip_gemm.h strip_mma16x6, strip_chain.h RingP3), from three-plane images of the TRANSPOSED weights; "0": fp32
    # matrix instructions
    BWD_SPLIT = True
    # ... in the N-split build (csrc/sasrec_strip_px.hip: eight waves per 64-row tile, two per SIMD, each owning half the output columns; the
    # entry points' products mode 4) wherever the strips run on three pieces: D 128, dropout 0.5 -- whatever the fold switches say.  One bit
    # per launch, top down: 1 = layer 1's feed-forward chain, 2 = layer 1's q / k / v chain + layer 0's feed-forward chain, 4 = layer 0's
    # q / k / v chain (+ the embedding backward); 0: the strip build everywhere (`bench.py --set STRIP_NSPLIT=0`, profiles/strip_nsplit.md)
    STRIP_NSPLIT = 7

    def _strip_mode(self, bf: int, launch: int) -> int:
        """The products mode of backward strip launch `launch` (0, 1, 2 top down) of a step whose strips take mode `bf`."""
        return 4 if bf == 3 and self.D == 128 and SASREC_P_DROP == 0.5 and (int(self.STRIP_NSPLIT) >> launch) & 1 else bf

    # ------------------------------------------------------------------ launch sequences
    def enqueue_prepare(self, pl: SasrecPlan, sparse: bool, bump_step: bool = False, defer_sort: bool = False) -> None:
        """defer_sort: only mark the fork point; the caller launches the sort with enqueue_sort() AFTER the main stream's next
        kernel.  (In the captured graph the branch that is enqueued first is dispatched first: with the sort ahead of the catch-up
        kernel the latter started ~20 us late in every replay.)"""
        L, s, shp = lib(), self.s, pl.shape
        # a train step (bump_step) of a loss that masks the other domain of every sample: the batch's live-sequence list
        # (amid_live_list_i32) rides in the packing launch; enqueue_forward then finds it in place (pl.live_packed)
        with_live = bool(bump_step and getattr(pl, "strip", False) and not self.itc_bs)
        pl.live_packed = with_live
        # ... and then sort, segment reduce and row Adam run on the live sequences' positions only (the dead sequences' gradient rows
        # are exact zeros; a row only they hold is not touched this step -- the lazy Adam replays it when it is next read).  InnerComp
        # couples the rows of a batch in front of the encoders: every position keeps its gradient there.
        pl.compact = bool(with_live and sparse and self.compact_ok(pl))
        # ... and the step's index sort rides in main-stream launches (catch-up + the three strip backward launches carry one phase
        # each as extra workgroups: no side stream, no fork, no join) when the keys fit the riders' 1024-bin build
        pl.riding = bool(bump_step and sparse and defer_sort and self.SORT_RIDERS and getattr(pl, "strip", False) and not pl.compact
                         and not self._seq_backward(pl)             # (the fused backward is one launch: three of the riders' hosts are gone)
                         and (shp.n_idx + 2047) // 2048 <= 2 * shp.Tenc and self._sort_plan(pl) is not None)
        # ... or, for the steps without five launches to ride in (the one-launch backward at T <= 32, BERT4Rec, the comp modules): the WHOLE sort
        # chained inside the catch-up launch (amid_lazy_adam_catchup_positions_sort_f32 phase 6) -- no side stream, no fork, no join
        pl.chain = bool(bump_step and sparse and defer_sort and self.SORT_CHAIN and not pl.riding and not pl.compact
                        and shp.n_idx <= lib().value("amid_sort_chain_max_indices") and self.n_rows <= (1 << 20) and self._sort_plan(pl) is not None)
        ent = self.input_pool(pl)
        # compute = "bf16": the step folds like the fp32 one when its shape does (the decisions below then see "f32": _ceff)
        self._bf16_as_f32 = False
        if self.compute == "bf16" and self.BF16_FOLD and bump_step and shp.B <= self.BF16_FOLD_MAX_B:
            self._bf16_as_f32 = True
            if not (ent is not None and sparse and defer_sort and with_live and self._tail2_ok(pl)):
                self._bf16_as_f32 = False
            else:
                pl.riding = False            # (decided above with the mode's own launches in mind: the folded step rides on the compact list's plan)
        # the live-sequence step on an input pool in twelve launches (FUSED_TAIL): packing, catch-up and phase 1 of the sort of the COMPACT
        # index list are one launch; the later phases ride in the backward strips and the weight gradients; no embedding-backward launch
        pl.tail2 = bool(ent is not None and bump_step and sparse and defer_sort and with_live and self._tail2_ok(pl))
        pl.gather_on_fwd = False
        pl.prepared = False
        if pl.tail2:
            self._ensure_opt_state()
            head = (self._marshal(pl), self._pool_batch(ent), self._adam_rows(),
                    dict(D=self.D, step_state=self.step_state.data_ptr(), sort_plan=self._sort_plan_c(pl), stream=s))
            # the step's gather as the prologue of its forward (amid_sas_seq_fwd_gather_*_f32): K1's riders -- the weight images of the forward
            # and of the backward strips -- move to this launch's last workgroups
            pl.gather_on_fwd = bool(self.GATHER_ON_FWD and self._fwd_on_pieces(pl, shp.B, shp.Tenc) and self._p3_bwd_for(pl) and shp.T == shp.Tenc)
            # a pool prepared at pool fill (PREPARED_POOL, engine_io.py): the head copies the batch's slab -- lists, sort, runs -- into the plan's
            # buffers instead of building it, and the four later launches that hosted the sort's phases 2 .. 5 run without riders
            slabs = self.pool_slabs(pl)
            pl.prepared = bool(self.PREPARED_POOL and slabs is not None and getattr(self, "_in_train_step", False) and self.compute != "bf16")
            if pl.prepared:
                L.call_named("amid_step_head_prepared_f32", *head, self._w16_riders() if pl.gather_on_fwd else NO_W16_RIDERS,
                             slab=slabs[0].data_ptr(), slab_stride=slabs[0].stride(0))
            elif pl.gather_on_fwd:
                L.call_named("amid_step_head_w16_f32", *head, self._w16_riders())
            else:
                L.call_named("amid_step_head_f32", *head)
            self.step += 1
            pl.compact, pl.riding, pl.chain = True, not pl.prepared, False
            self._sort_owed = False
            return
        st = self.step_state.data_ptr()
        if ent is not None:
            if not bump_step:
                raise ValueError("an input pool advances with the step counter: enqueue_prepare(bump_step=True) only")
            # (the marshal's table holds the live list: the form without one is not given it by a name it does not have)
            L.call_named("amid_pack_indices_pool_live" if with_live else "amid_pack_indices_pool", self._marshal(pl), self._pool_batch(ent),
                         step_state=st, stream=s)
            self.step += 1
            self._sort_behind_pack(pl, sparse, defer_sort)
            return
        L.call_named("amid_pack_indices_live" if with_live else "amid_pack_indices", self._marshal(pl), step_state=st if bump_step else None, stream=s)
        if bump_step:
            self.step += 1
        self._sort_behind_pack(pl, sparse, defer_sort)

    @staticmethod
    def _pool_batch(ent):
        """The batch an input pool's step reads: (pool, phase) under the header's names."""
        pool, phase = ent
        return dict(pool=pool.data_ptr(), pool_stride=pool.stride(0), n_pool=pool.shape[0], phase=phase)

    def _sort_behind_pack(self, pl: SasrecPlan, sparse: bool, defer_sort: bool) -> None:
        """The step's index sort once the packing launch is enqueued: riding in later launches, or forked onto the side stream here
        (defer_sort: by the caller, behind the main stream's next kernel)."""
        if sparse and (pl.riding or pl.chain):
            self._sort_owed = False
        elif sparse:
            self.ev_idx.record(self.stream)       # fork point: the index list is complete
            self._sort_owed = bool(defer_sort)
            if not defer_sort:
                self.enqueue_sort(pl)

    def enqueue_sort(self, pl: SasrecPlan) -> None:
        """Sort / unique on the side stream (joined by the gradient tail just before the segment reduce)."""
        L, shp = lib(), pl.shape
        self.side.wait_event(self.ev_idx)
        if getattr(pl, "compact", False):
            L.call("amid_sort_unique_rows_i32", pl.idx_c.data_ptr(), pl.row_c.data_ptr(), pl.n_compact, self.n_rows, pl.sort_ws.data_ptr(),
                   pl.pos_sorted.data_ptr(), pl.uniq_ids.data_ptr(), pl.seg_off.data_ptr(), pl.seg_of.data_ptr(), pl.n_uniq.data_ptr(),
                   self.side.cuda_stream)
        else:
            L.call("amid_sort_unique_i32", pl.idx_all.data_ptr(), shp.n_idx, self.n_rows, pl.sort_ws.data_ptr(), pl.pos_sorted.data_ptr(),
                   pl.uniq_ids.data_ptr(), pl.seg_off.data_ptr(), pl.seg_of.data_ptr(), pl.n_uniq.data_ptr(), self.side.cuda_stream)
        self.ev_sorted.record(self.side)
        self._sort_pending = True
        self._sort_owed = False

    def _wgrad_mode(self, D: int) -> int:
        """The mma mode of amid_sas_wgrad(_rows)_f32: 1 = operands rounded to bf16 (compute "bf16"), 2 / 3 = fp32 operands as three bf16
        pieces (nine / six piece pairs), 0 = fp32 matrix instructions."""
        if D != 128:
            return 0
        if self.BF16_WGRAD and getattr(self, "_bf16_bwd", False):
            return 1
        if self._bf16_as_f32 and self.BF16_WGRAD and self.BF16_FWD_ONE and getattr(self, "_wgrad_one", False):
            return 4                    # (the folded bf16 step's weight-gradient launch: ONE piece per operand -- asked for at the launch site only)
        return {"9": 2, "6": 3}.get(self.WGRAD_SPLIT, 0)

    def join_sort(self) -> None:
        """Make the main stream wait for the side-stream sort (no-op if nothing is pending)."""
        if getattr(self, "_sort_pending", False):
            self.stream.wait_event(self.ev_sorted)
            self._sort_pending = False

    SORT_RIDERS = True
    # compute = "bf16" on a step that folds (round 6): the fp32 step's nine launches -- its forward on bf16 pieces included, which is MORE than the mode
    # asks for -- with the backward strips' data-gradient products on ONE bf16 piece (they read the hi plane of the three-plane images).  Decided per
    # step in enqueue_prepare (_bf16_as_f32); BF16_FOLD_MAX_B: batches beyond it keep the unfolded bf16 launches.
    BF16_FOLD = True
    BF16_FOLD_MAX_B = 1 << 30          # (with the forward on one piece too the fold wins at B 512 as well: cfg 3 bf16 0.4915 -> 0.4751)
    BF16_FWD_ONE = True          # ... and its forward multiplies ONE piece per operand too (amid_sas_seq_fwd_gather_*_p1_f32): bf16 products
    _bf16_as_f32 = False

    def _ceff(self) -> str:
        """The compute mode the step's path decisions see: "f32" for a compute = "bf16" step that takes the folded launches."""
        return "f32" if self._bf16_as_f32 else self.compute
    FOLD_SHORT = True            # 16 < T <= 32 on an input pool: the folded strips step instead of the one-launch backward (round 6)
    # the whole sort chained inside the catch-up launch where the riders have no five launches (round 6).  Off by default: the chain takes ~ 45 us
    # (five phases, four barriers with agent-scope fences), which the catch-up hides only when it replays long gaps -- cfg 4's real epoch in its
    # steady state 0.2383 -> 0.2331 ms, but + 17 % on a T 20 step without lagging rows and + 5 % on BERT4Rec (DESIGN_HISTORY.md, "Round 6")
    SORT_CHAIN = False
    # compute = "bf16": the weight gradients' products on the bf16 matrix cores too (amid_sas_wgrad_rows_f32 mma_bf16); 0: fp32 products
    BF16_WGRAD = True
    # compute = "fp32": the weight gradients' products on the bf16 matrix cores at fp32 accuracy -- every operand element as three bf16
    # pieces, six ("6", the default) or nine ("9") piece pairs (csrc/sasrec_bwd.hip sas_wgrad_split_kernel; D = 128); "0": fp32 matrix
    # instructions.  Error against the fp64 product 3.8e-7 of the largest entry either way, 4.4e-7 for the fp32 instructions.
    WGRAD_SPLIT = "6"
    # compute = "fp32": the one-launch forward's twelve projections on the bf16 matrix cores at fp32 accuracy too (three bf16 pieces per
    # operand, six piece pairs; the pieces are made once, by the wave that produced the operand, and cross the strip's column parts as
    # operand fragments: amid_sas_seq_fwd_split_f32, csrc/sasrec_seqn.hip seqn_fwd_px_kernel; weight images by the gather's extra
    # workgroups).  Every saved tensor within 3e-6 of the fp32 build's; 153 k cycles against 187 k, step 0.3562 -> 0.3510 ms at cfg 2 (the
    # bf16-dense kernel runs at a lower clock: 15 % fewer cycles, 7 % less time).  "0": fp32 matrix instructions.
    FWD_SPLIT = True
    # The train step's encoder backward (data gradients) as ONE launch over the live sequences where csrc/sasrec_strip.hip covers the
    # shape (amid_sas_seq_bwd_f32): "auto" = where it wins.  It tiles one sequence per workgroup, a whole CU each, so the step's sort
    # riders find no free CU in it and the sort goes back to the side stream (a fork and a join, ~10 us of a replayed graph).  Measured
    # (MI355X, T 50): B 256 = one round of workgroups either way, a tie (0.391 against 0.389 ms with the riders); B 512 = two full
    # rounds against 400 row tiles in two uneven ones, 0.690 against 0.740 ms; B 4096 = 16 rounds against 12.5 rounds of denser row
    # tiles, 4.75 against 4.48 ms.  So: more live sequences than CUs, at most two rounds.  T <= 32 (csrc/sasrec_seqn_bwd.hip: two strips x
    # four column parts per sequence): B 256, T 20 runs 80 strip tiles per launch on 256 CUs -- 111 us in five launches against 67.8 in one,
    # 0.267 -> 0.243 ms per step with the sort back on its side stream; taken for B <= n_CU.  SEQ_BACKWARD = "1" / "0" forces it on / off.
    SEQ_BACKWARD = "auto"

    def _seq_backward(self, pl: SasrecPlan) -> bool:
        if not getattr(pl, "seq_bwd", False) or self.itc_bs or self.SEQ_BACKWARD in ("0", False):
            return False
        if self.SEQ_BACKWARD in ("1", True):
            return True
        n_cu = torch.cuda.get_device_properties(self.device).multi_processor_count
        if pl.shape.Tenc <= 32:         # short sequences: the strip launches fill a third of the chip, a workgroup per sequence all of it
            # ... unless the step folds (round 6; 16 < T: the head rides on the forward's tail): the strips host the riders, the gather and the
            # embedding backward ride too and no side stream forks -- cfg 4's real epoch 238.4 -> 229 us per step (profiles/tools/trace_cfg4.sh)
            if self.FOLD_SHORT and pl.shape.Tenc > 16 and self.D == 128 and self._folded_step_shape(pl):
                return False
            return pl.shape.B <= n_cu
        if self.D != 128:               # D 64 at T 50: the five strip launches win (B 512: 0.352 against 0.393 ms; B 256: a tie)
            return False
        if self._folded_step_shape(pl):      # the strips host the folded step's riders (round 5; cfg 3, B 512: 0.6006 against 0.6144 ms
            return False                    # for the one-launch backward in front of the fifteen-launch tail)
        return n_cu < pl.shape.B <= 2 * n_cu

    def _sort_plan(self, pl: SasrecPlan):
        """Host address of the plan of the step's index sort (amid_sort_plan_pack), or None when the riders do not cover it."""
        if not hasattr(pl, "_sort_plan_buf"):
            L = lib()
            buf = (ctypes.c_ubyte * L.value("amid_sort_plan_bytes"))()
            rc = L._fn["amid_sort_plan_pack"](ctypes.addressof(buf), pl.idx_all.data_ptr(), None, pl.shape.n_idx, self.n_rows,
                                              pl.sort_ws.data_ptr(), pl.pos_sorted.data_ptr(), pl.uniq_ids.data_ptr(), pl.seg_off.data_ptr(),
                                              pl.seg_of.data_ptr(), pl.n_uniq.data_ptr())
            pl._sort_plan_buf = buf if rc == 0 else None
        return ctypes.addressof(pl._sort_plan_buf) if pl._sort_plan_buf is not None else None

    def _sort_plan_c(self, pl: SasrecPlan):
        """Host address of the sort plan over the plan's COMPACT list (idx_c, row_c), or None when the riders do not cover it."""
        if not hasattr(pl, "_sort_plan_c_buf"):
            L = lib()
            buf = (ctypes.c_ubyte * L.value("amid_sort_plan_bytes"))()
            rc = L._fn["amid_sort_plan_pack"](ctypes.addressof(buf), pl.idx_c.data_ptr(), pl.row_c.data_ptr(), pl.n_compact, self.n_rows,
                                              pl.sort_ws.data_ptr(), pl.pos_sorted.data_ptr(), pl.uniq_ids.data_ptr(), pl.seg_off.data_ptr(),
                                              pl.seg_of.data_ptr(), pl.n_uniq.data_ptr())
            pl._sort_plan_c_buf = buf if rc == 0 else None
        return ctypes.addressof(pl._sort_plan_c_buf) if pl._sort_plan_c_buf is not None else None

    # The live-sequence train step on an input pool with its head and tail folded (round 5): amid_step_head_f32 (packing + catch-up + sort
    # phase 1 over the compact list), the embedding backward on the last strip launch (amid_sas_strip_qkv_bwd_emb_f32), the sort's last
    # phase in the weight-gradient launch, the position rows' gradients in the gradient tail (amid_grad_tail_live_f32) and the segment
    # reduce's second phase in the optimizer launch (amid_optimizer_step_spans_f32): 12 launches instead of 15.  False: round 4's sequence
    # (tests compare the two).
    FUSED_OPT = True             # the folded step's optimizer inside its gradient tail: ten launches (round 6; False: eleven)
    GATHER_ON_FWD = True         # ... and its gather K1 as the prologue of the forward's workgroups: nine (the weight images by the step head's riders)
    FUSED_SPANS = True           # every single-GPU train step: the segment reduce's second phase inside the optimizer launch (round 5)
    FUSED_TAIL = True
    # The folded single-GPU step on a pool PREPARED at pool fill (csrc/pool_prepare.hip; set_input_pool / refill_input_pool make one slab per
    # batch: index lists, live list, the stable sort of the compact list and its runs -- all functions of the batch alone): the step head
    # copies its batch's slab instead of building it (amid_step_head_prepared_f32) and the sort's phases 2 .. 5 leave the strips and the
    # weight-gradient launch.  Tables of up to 2^20 rows; data parallel, bf16 and the other models keep the per-step path.  False: the
    # step is bit for bit the per-step one (tests/test_gpu_prepared_pool.py; `bench.py --set PREPARED_POOL=0`).
    PREPARED_POOL = True

    def _coll(self, fn) -> None:
        """A collective in the MIDDLE of a step (InterComp's / InnerComp's gathers and reductions under data parallel).  Eagerly: run it.
        While engine_dp captures the step in segments (_seg_capture: a list), a collective cannot sit inside a captured graph: the capture
        ends here, the graph so far and the collective are recorded in order, and a new capture begins behind it -- the replay launches
        graph | collective | graph | ... (engine_dp.train_step_dp)."""
        seg = getattr(self, "_seg_capture", None)
        if seg is None:
            fn()
            return
        L = lib()
        if getattr(self, "_sort_owed", False):      # a deferred side-stream sort whose fork point has not come yet: start it now ...
            self.ev_idx.record(self.stream)
            self.enqueue_sort(self._seg_plan)
        self.join_sort()                            # ... and join it: a capture cannot end with forked work (the segment then holds the whole sort)
        out = ctypes.c_void_p()
        L.call("amid_graph_capture_end", self.s, ctypes.byref(out))
        try:
            seg.append(("graph", out.value))
            seg.append(("call", fn))
        finally:      # the caller's `finally` ends a capture: the stream is capturing again whatever happened in between
            L.call("amid_graph_capture_begin", self.s)

    # The data-parallel step's local half (enqueue_local_grads: graph A of the graph pair, the local-gradients graph, the eager step) in the
    # folded form too (round 6): step head, head on the forward's tail, embedding backward on the last strip, position rows in the tail; phase B
    # of the segment reduce stays a launch (with the chunk's packing riding in it) because the exchange ships the finished rows.
    FUSED_TAIL_DP = True

    def _fold_ctx(self) -> bool:
        """Whether the launches being enqueued belong to a step that may take the folded form."""
        return bool(getattr(self, "_in_train_step", False) or (getattr(self, "_in_local_grads", False) and self.FUSED_TAIL_DP))

    def _folded_step_shape(self, pl: SasrecPlan) -> bool:
        """The conditions of the folded twelve-launch step that do not depend on how the backward runs (_tail2_ok adds those)."""
        return bool(self.FUSED_TAIL and self._fold_ctx() and self.SORT_RIDERS and pl.need_grad and self.D == 128
                    and self._ceff() == "f32" and not self.dr and not self.itc_bs and not self.inc_bs and not getattr(self, "comp", "")
                    and 1 < pl.shape.NI <= 64 and self.FUSED_HEAD and self.BWD_SPLIT and pl.strip      # (the head's hidden-gradient form: one item chunk)
                    and self.input_pool(pl) is not None and self.live_forward_ok(pl) and self._wgrad_mode(self.D) == 3
                    and not self._fold_catchup(pl) and self._sort_plan_c(pl) is not None and (pl.n_compact + 2047) // 2048 <= 12 * pl.splits)

    def _tail2_ok(self, pl: SasrecPlan) -> bool:
        shp = pl.shape
        # (inside enqueue_train_step the segment reduce's runs across chunks are finished by THIS step's optimizer launch; inside
        # enqueue_local_grads -- what a data-parallel exchange ships -- by a launch of their own behind the tail, amid_grad_tail_live_dp_f32)
        return bool(self.FUSED_TAIL and self._fold_ctx() and self.SORT_RIDERS and pl.need_grad and self.D == 128 and self._ceff() == "f32" and not self.dr
                    and not self.itc_bs and not self.inc_bs and not getattr(self, "comp", "") and 1 < pl.shape.NI <= 64
                    and self.FUSED_HEAD and self.live_forward_ok(pl) and self._p3_bwd_for(pl) and self._wgrad_mode(self.D) == 3
                    and not self._fold_catchup(pl) and self._sort_plan_c(pl) is not None
                    and (pl.n_compact + 2047) // 2048 <= 12 * pl.splits)

    def _tail2_table(self, pl: SasrecPlan):
        """The gradient tail's reduce table without the position rows' partial sums and without the scorer's per-sample partials
        (amid_grad_tail_live_f32 sums the former from the rows and forms the latter from the head's per-sample hidden gradients)."""
        if not hasattr(pl, "red_entries_t"):
            pl.red_entries_t, pl.red_n_t, pl.red_max_t = pl._build_reduce_table(self, live=True, pos=False)
        return pl.red_entries_t, pl.red_n_t, pl.red_blk_t

    def _ln_stat(self, pl: SasrecPlan):
        """(tensors, host pointer array) of the per-layer row statistics [2 M][4] a forward stores instead of qn / y."""
        if not hasattr(pl, "ln_stat"):
            pl.ln_stat = [torch.zeros(2 * pl.shape.M, 4, dtype=torch.float32, device=self.device) for _ in range(2)]
            pl._ln_stat_ptrs = ptr_array([t.data_ptr() for t in pl.ln_stat])
            torch.cuda.synchronize(self.device)      # zero-filled on torch's stream, used on the engine's
        return pl.ln_stat, pl._ln_stat_ptrs

    def _hidg(self, pl: SasrecPlan) -> torch.Tensor:
        if not hasattr(pl, "hidg"):
            pl.hidg = torch.zeros(pl.shape.B, lib().value("amid_scorer_vec_floats", pl.shape.NI, self.hid), dtype=torch.float32, device=self.device)
            torch.cuda.synchronize(self.device)
        return pl.hidg

    COMPACT_LIVE = True
    COMPACT_MIN_IDX = 65536    # shorter index lists gain nothing from the compact list (the tail is bound by the dense partial sums,
                               # the row Adam by its dense half) and lose the early fork of the side-stream sort: cfg 2 keeps the full list

    def live_forward_ok(self, pl: SasrecPlan) -> bool:
        """Whether this engine's train step on `pl` encodes the live sequences only (see _enqueue_fwd_bwd)."""
        return bool(getattr(pl, "strip", False) and not self.itc_bs and not self.dr and not self.inc_bs and self.FUSED_HEAD and self.LIVE_FORWARD
                    and self.loss == "bce"      # (a listwise step's head reads the user vectors of a launch of its own: every sequence is encoded)
                    and lib().value("amid_attn_live_supported", pl.shape.Tenc, self.D, self.H, 1))

    def n_sparse_train(self, pl: SasrecPlan, dp: bool = False) -> int:
        """n_sparse() of this engine's train steps on `pl` (known before the step is enqueued); dp: of its data-parallel steps."""
        if self.compact_ok(pl):
            return pl.n_compact
        flag = "_in_local_grads" if dp else "_in_train_step"      # (the folded step forces the compact list whatever the index count)
        saved = getattr(self, flag, False)
        setattr(self, flag, True)
        try:
            folded = self.input_pool(pl) is not None and self._tail2_ok(pl)
        finally:
            setattr(self, flag, saved)
        return pl.n_compact if folded else pl.shape.n_idx

    def compact_ok(self, pl: SasrecPlan) -> bool:
        return bool(self.COMPACT_LIVE and pl.shape.n_idx >= self.COMPACT_MIN_IDX and self.live_forward_ok(pl))

    def n_sparse(self, pl: SasrecPlan) -> int:
        """Entries of the step's index list as the sparse side (sort, segment reduce, row Adam) sees it."""
        return pl.n_compact if getattr(pl, "compact", False) else pl.shape.n_idx

    # The lazy-Adam catch-up of a step can be FOLDED into the gather K1 (amid_embed_fwd_replay_f32): a lagging row's owed zero-gradient steps
    # are replayed in registers for the value the forward reads, and once more by the optimizer launch (which replays lagging rows anyway)
    # in front of the real step -- one launch less, the replay done twice.  MEASURED (MI355X, cfg 2: ~2.5 k rows of a step lag by ~60 steps,
    # an epoch is 60 batches): the catch-up launch is not latency but replay arithmetic (two quarter-rate instructions per element and
    # step), so doing it twice LOSES -- catch-up 14.4 + K1 8.1 us -> K1 24.5 us, optimizer 7.4 -> 15.6 us, 0.3695 -> 0.3829 ms per step;
    # cfg 4 0.239 -> 0.268.  Off by default; "auto" folds only where the replay is next to nothing (an epoch of at most FOLD_MAX_GAP
    # batches, e.g. a handful of batches replayed over and over), "1" always.
    FOLD_CATCHUP = "0"
    FOLD_MAX_GAP = 8
    catchup_gap_hint: Optional[int] = None          # batches per epoch when no input pool says so (the CLI's per-batch path)

    def _fold_catchup(self, pl: SasrecPlan) -> bool:
        if self.inc_bs or getattr(self, "comp", "") or self.FOLD_CATCHUP in ("0", False):
            return False                             # (InnerComp / BERT4Rec comp gather with amid_gather_rows_f32: no replay there)
        if self.FOLD_CATCHUP in ("1", True):
            return True
        ent = self.input_pool(pl)
        gap = ent[0].shape[0] if ent is not None else self.catchup_gap_hint
        return gap is not None and gap <= self.FOLD_MAX_GAP

    def _w16_images(self, planes: int):
        """(host pointer array of the 24 encoder weights [layer][domain][q, k, v, o, conv1, conv2], the image buffer) for `planes` bf16
        planes per weight (1: operands rounded to bf16; 3: hi + mid + lo = the fp32 weight exactly)."""
        D = self.D
        # one buffer per plane count, never re-allocated: captured graphs hold these addresses, and a compute = "bf16" engine alternates between
        # three planes (its folded train step, round 6) and one (its evaluation forward)
        bufs = self.__dict__.setdefault("_w16_bufs", {})
        if planes not in bufs:
            bufs[planes] = torch.empty(2, 2, 6, planes, D * D, dtype=torch.bfloat16, device=self.device)
        self.w16 = bufs[planes]
        return self._wT_lists()[0], self.w16

    def _p3_bwd_for(self, pl: SasrecPlan) -> bool:
        """Whether this plan's backward strips take their data-gradient products on bf16 pieces (three-plane images of the transposes)."""
        return bool(self._ceff() != "bf16" and self.BWD_SPLIT and pl.strip and self.D == 128 and not self._seq_backward(pl))

    def _wT16x3_buf(self):
        if not hasattr(self, "wT16x3"):
            self.wT16x3 = torch.empty(2, 2, 6, 3, self.D * self.D, dtype=torch.bfloat16, device=self.device)
        return self.wT16x3

    def _fwd_on_pieces(self, pl: SasrecPlan, B: int, T: int) -> bool:
        """Whether this step's encoder forward is the one-launch kernel with its products on bf16 pieces (amid_sas_seq_fwd_split_f32)."""
        return bool(self._ceff() != "bf16" and self.FWD_SPLIT and self.D == 128 and pl.strip and self.SEQ_FORWARD and not self.inc_bs
                    and lib().value("amid_sas_seq_supported", B, T, self.D, self.H))

    def _enqueue_k1(self, pl: SasrecPlan, pos0, pos1, tmq, tr: int, p_drop: float, lf, items: bool = True) -> None:
        """The gather K1 of a forward in the variant the step needs: over every sequence or the live list `lf`, writing the compact index
        list, with the folded catch-up (+ phase 1 of a riding sort).  items=False: the sequences' rows only (the evaluation head gathers
        the candidates' rows itself)."""
        L, shp = lib(), pl.shape
        B, T, NI = shp.B, shp.Tenc, shp.NI if items else 0
        st = self.step_state.data_ptr()
        # what this launch's riders write is decided HERE: a flag left by an earlier forward (e.g. a train-mode forward without a backward)
        # must not make the next backward skip its images
        pl.w16_written = pl.wT16x3_written = False
        compact = lf is not None and getattr(pl, "compact", False) and not getattr(pl, "tail2", False)      # (tail2: the step head wrote the list)
        ic, rc = (pl.idx_c.data_ptr(), pl.row_c.data_ptr()) if compact else (None, None)
        k1, table = self._k1_head(pl, pos0, pos1, tmq, tr, p_drop, B * NI), self.table.data_ptr()
        if getattr(pl, "fold_catchup", False):
            pl.fold_catchup = False
            ride = getattr(pl, "riding", False)
            # (the step state twice: the dropout counters' as every K1 form takes it, and the replay's Adam coefficients under a name of its own)
            L.call_named("amid_embed_fwd_replay_f32", self._adam_rows(), k1, live=lf, idx_c=ic, row_c=rc, adam_state=st,
                         sort_plan=self._sort_plan(pl) if ride else None, sort_phase=1 if ride else 0)
        elif self._fwd_on_pieces(pl, B, T):          # the gather's extra workgroups write this step's weight images (three bf16 planes each)
            wt = bool(tr and self._p3_bwd_for(pl))       # (+ the transposes' images for this step's backward strips)
            L.call_named("amid_embed_fwd_w16_f32", k1, self._w16_riders(transposes=wt), table=table, live=lf, idx_c=ic, row_c=rc)
            pl.w16_written = True
            pl.wT16x3_written = wt
        elif compact:
            L.call_named("amid_embed_fwd_live_compact_f32", k1, table=table, live=lf, idx_c=ic, row_c=rc)
        elif lf is not None:
            L.call_named("amid_embed_fwd_live_f32", k1, table=table, live=lf)
        else:
            L.call_named("amid_embed_fwd_f32", k1, table=table)
        if getattr(self, "_sort_owed", False):      # a deferred side-stream sort starts behind K1 (the compact list is K1's by-product; with
            if compact:                              # the folded catch-up the fork waited so that the main branch is captured first)
                self.ev_idx.record(self.stream)
            self.enqueue_sort(pl)

    def enqueue_catchup(self, pl: SasrecPlan) -> None:
        """Replay pending zero-gradient Adam steps of the rows this batch is about to gather (by position: no sort needed) -- as a
        launch of its own, or folded into the gather that follows (_fold_catchup)."""
        self._ensure_opt_state()
        if getattr(pl, "tail2", False):           # the step head replayed them
            pl.fold_catchup = False
            return
        chain = getattr(pl, "chain", False)
        pl.fold_catchup = self._fold_catchup(pl) and not chain       # (the chain rides in the catch-up's own launch)
        if pl.fold_catchup:
            return
        at = dict(idx=pl.idx_all.data_ptr(), n_idx=pl.shape.n_idx, D=self.D, step_state=self.step_state.data_ptr(), stream=self.s)
        if chain:                                 # the step's whole sort rides here (five phases, the riders' own barrier between them)
            lib().call_named("amid_lazy_adam_catchup_positions_sort_f32", self._adam_rows(), at, sort_plan=self._sort_plan(pl), sort_phase=6)
            return
        if getattr(pl, "riding", False):          # phase 1 of the step's sort rides here
            lib().call_named("amid_lazy_adam_catchup_positions_sort_f32", self._adam_rows(), at, sort_plan=self._sort_plan(pl), sort_phase=1)
            return
        lib().call_named("amid_lazy_adam_catchup_positions_f32", self._adam_rows(), at)

    def enqueue_forward(self, pl: SasrecPlan, train: bool, with_loss: bool, sum_loss: bool = True, head: bool = True, gather_items: bool = True) -> None:
        """head=False: stop behind the encoders (pl.x[2] is the last layer's output); gather_items=False: the candidates' rows are not gathered
        (enqueue_eval: its head reads them from the table)."""
        L, s, shp, D = lib(), self.s, pl.shape, self.D
        B, T, NI, M = shp.B, shp.Tenc, shp.NI, shp.M
        st = self.step_state.data_ptr()
        tr = 1 if train else 0
        fp = self.dense
        pl.w16_written = pl.wT16x3_written = False      # (set again by the gather K1 of THIS forward when its riders write the images)
        pl.head_done = False                            # (set by THIS forward when its workgroups run the head: HEAD_ON_FWD)
        pl.lnstat_fwd = False                           # (set by THIS forward when it stores row statistics instead of qn / y)
        # the train step's own loss reads only the sequence (domain_id[b], b) of every sample (see _enqueue_fwd_bwd): those B "live"
        # sequences are listed on the device; with live_fwd the forward encodes nothing else
        lv = self._live_list(pl)
        live_fwd = lv is not None and getattr(self, "_live_fwd", False)
        lf = lv if live_fwd else None
        if lv is not None and not getattr(pl, "live_packed", False):
            L.call("amid_live_list_i32", pl.domain.data_ptr(), B, pl.live.data_ptr(), s)
        if self.inc_bs:      # plain gather, InnerComp's token group, then the 2T-token encoder input (csrc/innercomp.hip)
            L.call("amid_gather_rows_f32", self.table.data_ptr(), self.n_rows, D, pl.idx_all.data_ptr(), 0, shp.n_idx if gather_items else 2 * shp.Mi,
                   pl.xg.data_ptr(), None, s)
            L.call("amid_inc_score_f32", pl.xg.data_ptr(), B, shp.T, D, pl.inc_s.data_ptr(), s)
            wts = (self._pp("inc_d{d}.trans_nn.weight"), self._pp("inc_d{d}.trans_nn.bias"), self._pp("inc_d{d}.trans_bs.weight"),
                   self._pp("inc_d{d}.trans_bs.bias"))
            out = (pl.inc_gate.data_ptr(), pl.inc_S.data_ptr(), pl.inc_Z.data_ptr(), pl.inc_sw.data_ptr(), pl.x[0].data_ptr(),
                   pl.tmq.data_ptr(), st, tr, SASREC_P_DROP, s)
            if getattr(pl, "inc_world", 1) > 1:
                # data parallel: the softmax over the batch and Linear(bs, 1) span the GLOBAL batch (model_seq.py:465-469).  The ranks
                # all-gather their scores (per domain, rank order = sample order), each forms the gates of its own rows and its partial
                # token sums S, the partial sums are all-reduced, and every rank finishes Z -- the same group on every rank
                ex = self._inc_exchange(pl)
                self._coll(lambda: [ex.all_gather_packed(pl.inc_s[g], pl.inc_s_g[g]) for g in (0, 1)])
                shard = (B, shp.T, D, self.inc_bs, ex.rank * B)
                L.call("amid_inc_embed_fwd_shard_f32", pl.xg.data_ptr(), pl.inc_s_g.data_ptr(), *wts, self.inc_threshold,
                       fp.ptr("sac1.pos_emb.weight"), fp.ptr("sac2.pos_emb.weight"), *shard, 1, *out)
                self._coll(lambda: ex.all_reduce_dense(pl.inc_S))
                L.call("amid_inc_embed_fwd_shard_f32", pl.xg.data_ptr(), pl.inc_s_g.data_ptr(), *wts, self.inc_threshold,
                       fp.ptr("sac1.pos_emb.weight"), fp.ptr("sac2.pos_emb.weight"), *shard, 2, *out)
            else:
                L.call("amid_inc_embed_fwd_f32", pl.xg.data_ptr(), pl.inc_s.data_ptr(), *wts, self.inc_threshold,
                       fp.ptr("sac1.pos_emb.weight"), fp.ptr("sac2.pos_emb.weight"), B, shp.T, D, *out)
        else:
            gat = bool(getattr(pl, "gather_on_fwd", False) and getattr(pl, "tail2", False) and lf is not None and tr)
            pl.gather_on_fwd = False                    # (a decision of THIS step's enqueue_prepare)
            if gat:                                     # the forward's workgroups gather their own rows; the step head wrote the images
                pl.w16_written = pl.wT16x3_written = True
            else:
                self._enqueue_k1(pl, fp.ptr("sac1.pos_emb.weight"), fp.ptr("sac2.pos_emb.weight"), pl.tmq.data_ptr(), tr, SASREC_P_DROP, lf, gather_items)
        lay = self._lay()
        att = dict(B=B, T=T, D=D, H=self.H, causal=1, step_state=st, train=tr, p_drop=SASREC_P_DROP, stream=s)

        def attn_fwd(l):
            if live_fwd:
                L.call_named("amid_attn_fwd_live_f32", self._saved(pl, l), att, layer=l, live=lf)
            else:
                L.call_named("amid_attn_fwd_f32", self._saved(pl, l), att, layer=l, key_keep=None)

        # a layer's out-projection + feed-forward launch of the strip and row-tile forms: it computes the NEXT layer's LayerNorm + q / k / v
        # too (behind the last layer: an absent block)
        ffn = lambda l: (lay[l], self._saved(pl, l), self._qkv_block(pl, 1, "n") if l == 0 else NO_NEXT_QKV,      # noqa: E731
                         dict(ln_w=lay[l]["ln2_w"], ln_b=lay[l]["ln2_b"], layer=l, tmq=pl.tmq.data_ptr(), step_state=st, train=tr, p_drop=SASREC_P_DROP))

        if pl.strip and self.SEQ_FORWARD and not self.inc_bs and L.value("amid_sas_seq_supported", B, T, D, self.H):
            # the whole encoder -- both layers, attention cores included -- as ONE launch, a workgroup per sequence (csrc/sasrec_seq.hip)
            sv, fams = self._seq_ptrs(pl), self._fams()
            # what every form of it takes (the folded forms take ln_stat where the others take qn, and no y: sv's qn / y are then not bound)
            enc = dict(n_layers=2, tmq=pl.tmq.data_ptr(), ln_eps=SASREC_LN_EPS, B=B, T=T, D=D, H=self.H, live=lf, step_state=st, train=tr,
                       p_drop=SASREC_P_DROP, stream=s)
            split = self._fwd_on_pieces(pl, B, T)
            if self._ceff() == "bf16" or split:       # this step's weights as bf16 fragment images (one plane: operands rounded to bf16;
                planes = 3 if split else 1            # three: hi + mid + lo = the fp32 weight exactly), then the forward on them
                src, w16 = self._w16_images(planes)
                if not getattr(pl, "w16_written", False):      # (the train step's gather K1 wrote them with extra workgroups)
                    L.call("amid_sas_weights_bf16_planes", src, 24, D, 0, planes, w16.data_ptr(), s)
                pl.w16_written = False
                if split and getattr(pl, "tail2", False) and lf is not None:
                    # the folded step: qn / y are not stored -- row statistics instead (pl.ln_stat); the weight gradients rebuild them
                    items = pl.xg.data_ptr() + 4 * 2 * shp.Mi * D
                    gather = dict(self._pos(), table=self.table.data_ptr(), idx_all=pl.idx_all.data_ptr())      # (the gather forms' prologue)
                    if (self.HEAD_ON_FWD and getattr(self, "_fuse_head", False) and with_loss and not sum_loss and 16 < T <= 64
                            and self.hid <= 32 and NI <= 64):
                        # ... and a live sequence is a sample: its workgroup finishes with the sample's head (forward + loss + backward,
                        # what amid_head_fwd_bwd_own_vec_f32 does in enqueue_backward otherwise); the last layer's output is not stored
                        # (compute = "bf16" on the folded step: the same launch multiplying ONE piece per operand, BF16_FWD_ONE)
                        p1 = "_p1" if (gat and self._bf16_as_f32 and self.BF16_FWD_ONE) else ""
                        L.call_named(f"amid_sas_seq_fwd_gather_head{p1}_f32" if gat else "amid_sas_seq_fwd_split_lnstat_head_f32", sv, fams, enc,
                                     gather, self._last_ln(("last_ln_w", "last_ln_b")), self._scorer(("sw1", "sb1", "sw2", "sb2")),
                                     xout=pl.x[2].data_ptr() if self.HEAD_ON_FWD_KEEPS_X else None, ln_stat=self._ln_stat(pl)[1],
                                     w16x3=w16.data_ptr(), items=items, labels=pl.labels.data_ptr(), domain_id=pl.domain.data_ptr(), NI=NI,
                                     hid=self.hid, u=pl.u.data_ptr(), p1=pl.p1.data_ptr(), p2=pl.p2.data_ptr(), dp1=pl.dp1.data_ptr(),
                                     dp2=pl.dp2.data_ptr(), loss_part=pl.loss_part.data_ptr(), dx=pl.dxbuf.data_ptr(),
                                     ditems=pl.dxg.data_ptr() + 4 * 2 * shp.Mi * D, ln_part=pl.last_part.data_ptr(),
                                     hidg=self._hidg(pl).data_ptr())
                        pl.head_done = True
                    elif gat:
                        p1 = "_p1" if (self._bf16_as_f32 and self.BF16_FWD_ONE) else ""
                        L.call_named(f"amid_sas_seq_fwd_gather{p1}_f32", sv, fams, enc, gather, xout=pl.x[2].data_ptr(),
                                     ln_stat=self._ln_stat(pl)[1], w16x3=w16.data_ptr(), items=items, NI=NI)
                    else:
                        L.call_named("amid_sas_seq_fwd_split_lnstat_f32", sv, fams, enc, xout=pl.x[2].data_ptr(), ln_stat=self._ln_stat(pl)[1],
                                     w16x3=w16.data_ptr())
                    pl.lnstat_fwd = True
                else:
                    pl.lnstat_fwd = False
                    if split:
                        L.call_named("amid_sas_seq_fwd_split_f32", sv, fams, enc, xout=pl.x[2].data_ptr(), w16x3=w16.data_ptr())
                    else:
                        L.call_named("amid_sas_seq_fwd_bf16w_f32", sv, fams, enc, xout=pl.x[2].data_ptr(), w16=w16.data_ptr())
            else:
                L.call_named("amid_sas_seq_fwd_f32", sv, fams, enc, xout=pl.x[2].data_ptr())
        elif pl.strip:       # register-resident strip chains (csrc/sasrec_strip.hip): same operations, operands and saved tensors
            dims = dict(ln_eps=SASREC_LN_EPS, B=B, T=T, D=D, live=lf, stream=s)
            L.call_named("amid_sas_strip_qkv_fwd_f32", self._qkv_block(pl, 0), dims, x=pl.x[0].data_ptr())
            attn_fwd(0)
            L.call_named("amid_sas_strip_oproj_ffn_fwd_f32", *ffn(0), dims)
            attn_fwd(1)
            L.call_named("amid_sas_strip_oproj_ffn_fwd_f32", *ffn(1), dims)
        else:
            dims = dict(ln_eps=SASREC_LN_EPS, M=M, D=D, rows_per_tile=pl.rpt, mma_bf16=self.mma_bf16, stream=s)
            L.call_named("amid_sas_qkv_fwd_f32" + pl.rt_suffix, self._qkv_block(pl, 0), dims, x=pl.x[0].data_ptr())
            for l in (0, 1):
                attn_fwd(l)
                if l == 0:      # layer 0's out-projection + feed-forward and layer 1's LayerNorm + q / k / v: one launch
                    L.call_named("amid_sas_oproj_ffn_qkv_fwd_f32" + pl.rt_suffix, *ffn(0), dims)
                else:
                    L.call_named("amid_sas_oproj_ffn_fwd_f32" + pl.rt_suffix, *ffn(l), dims)
        if not head:
            return
        if not gather_items:
            raise ValueError("enqueue_forward: the heads read the candidates' gathered rows (gather_items=False goes with head=False)")
        items = pl.xg.data_ptr() + 4 * 2 * shp.Mi * D
        if self._listwise_fwd(pl, with_loss, sum_loss):
            return
        if (self.dr or self.itc_bs) and getattr(self, "_fuse_scorers", False) and with_loss and not sum_loss:
            self._enqueue_user_vectors(pl)           # train step: the scorers run as ONE forward + loss + backward launch in enqueue_backward
            return
        if self.dr:
            self._enqueue_head_dr_fwd(pl, items, with_loss)
            return
        if self.itc_bs:
            self._enqueue_head_itc_fwd(pl, items, with_loss)
            if with_loss and sum_loss:
                L.call("amid_sum_vector_f32", pl.loss_part.data_ptr(), B, pl.loss.data_ptr(), s)
            return
        if getattr(self, "_fuse_head", False) and with_loss and not sum_loss:
            return                                   # train step: the head runs as ONE forward + backward launch in enqueue_backward
        L.call_named("amid_head_fwd_f32", self._last_ln(), self._scorer(), x=pl.x[2].data_ptr(), items=items,
                     labels=pl.labels.data_ptr() if with_loss else None, domain_id=pl.domain.data_ptr() if with_loss else None,
                     B=B, T=T, NI=NI, D=D, hid=self.hid, eps=SASREC_LN_EPS, u=pl.u.data_ptr(), p1=pl.p1.data_ptr(), p2=pl.p2.data_ptr(),
                     dp1=pl.dp1.data_ptr() if with_loss else None, dp2=pl.dp2.data_ptr() if with_loss else None,
                     loss_part=pl.loss_part.data_ptr() if with_loss else None, stream=s)
        if with_loss and sum_loss:
            L.call("amid_sum_vector_f32", pl.loss_part.data_ptr(), B, pl.loss.data_ptr(), s)

    # ---- isItC head: last LayerNorm + mean -> pair-max -> batch-softmax gate + mix -> scorer (csrc/intercomp.hip) ----
    def _enqueue_user_vectors(self, pl: SasrecPlan, mix: bool = True) -> None:
        """pl.u [2, B, D]: mean over time of the last LayerNorm (:385, :432-434), mixed with the InterComp group when isItC
        (mix=False: only the pair-max launch -- pl.itc_s and the unmixed pl.u_raw; the evaluation head mixes in its prologue)."""
        L, s, shp, D = lib(), self.s, pl.shape, self.D
        B, T = shp.B, shp.Tenc
        fp = self.dense
        if not self.itc_bs:
            L.call("amid_lnmean_fwd_f32", pl.x[2].data_ptr(), fp.ptr("sac1.last_layernorm.weight"), fp.ptr("sac1.last_layernorm.bias"),
                   fp.ptr("sac2.last_layernorm.weight"), fp.ptr("sac2.last_layernorm.bias"), B, T, D, SASREC_LN_EPS, pl.u.data_ptr(), s)
        else:            # the pair-max kernel has every LayerNorm'd row of (b) in LDS: it emits the means too
            L.call("amid_itc_pairmax_f32", pl.x[2].data_ptr(), self._pp("sac{d}.last_layernorm.weight"), self._pp("sac{d}.last_layernorm.bias"),
                   B, T, D, SASREC_LN_EPS, pl.itc_s.data_ptr(), pl.u_raw.data_ptr(), s)
            if not mix:
                return
            u_raw, itc_s, u_out, Bm = pl.u_raw, pl.itc_s, pl.u, B
            if pl.itc_world > 1:
                # data parallel: the module couples the rows of the GLOBAL batch (softmax over the batch model_seq.py:491, Linear(bs, 1)
                # over it :495).  Every rank gathers the shards' pair-max scalars and user vectors (rank r holds rows [r B, (r + 1) B)) and
                # evaluates the module on all bs rows -- the same arithmetic on the same values on every rank --, then keeps its rows.
                ex = self._itc_exchange(pl)
                self._coll(lambda: [ex.all_gather_packed(pl.u_raw[g].reshape(-1), pl.u_raw_g[g].reshape(-1)) for g in (0, 1)]
                           + [ex.all_gather_packed(pl.itc_s, pl.itc_s_g)])
                u_raw, itc_s, u_out, Bm = pl.u_raw_g, pl.itc_s_g, pl.u_g, self.itc_bs
            L.call("amid_itc_mix_fwd_f32", u_raw.data_ptr(), itc_s.data_ptr(), self._pp("itc_d{d}.trans_nn.weight"),
                   self._pp("itc_d{d}.trans_nn.bias"), self._pp("itc_d{d}.trans_bs.weight"), self._pp("itc_d{d}.trans_bs.bias"),
                   self.itc_threshold, Bm, D, pl.itc_gate.data_ptr(), pl.itc_z.data_ptr(), pl.itc_sw.data_ptr(), u_out.data_ptr(), s)
            if pl.itc_world > 1:
                r = self._itc_exchange(pl).rank
                pl.u.copy_(pl.u_g[:, r * B:(r + 1) * B])

    def _inc_exchange(self, pl: SasrecPlan):
        """The exchange of the running data-parallel step (train_step_dp) for a plan that holds a shard of InnerComp's global batch."""
        ex = getattr(self, "_dp_exchange", None)
        if ex is None or ex.world != pl.inc_world:
            raise ValueError(f"isInC: the batch must hold exactly bs = {self.inc_bs} rows (trans_bs is Linear(bs, 1) over the batch, "
                             f"model_seq.py:457); a batch of 1 / {pl.inc_world} of them is a data-parallel shard and can only be stepped by "
                             f"train_step_dp with an exchange over {pl.inc_world} ranks")
        return ex

    def _itc_exchange(self, pl: SasrecPlan):
        """The exchange of the running data-parallel step (train_step_dp) for a plan that holds a shard of InterComp's global batch."""
        ex = getattr(self, "_dp_exchange", None)
        if ex is None or ex.world != pl.itc_world:
            raise ValueError(f"isItC: the batch must hold exactly bs = {self.itc_bs} rows (trans_bs is Linear(bs, 1) over the batch, "
                             f"model_seq.py:480); a batch of 1 / {pl.itc_world} of them is a data-parallel shard and can only be stepped by "
                             f"train_step_dp with an exchange over {pl.itc_world} ranks")
        return ex

    def _enqueue_user_vectors_bwd(self, pl: SasrecPlan) -> None:
        """pl.du (gradient of pl.u) -> InterComp parameter gradients (isItC) -> dx of the last layer's output + LayerNorm partials."""
        L, s, shp, D = lib(), self.s, pl.shape, self.D
        B, T = shp.B, shp.Tenc
        fp, G = self.dense, self.dense.grad
        du = pl.du
        if self.itc_bs:
            du_in, u_raw, du_out, Bm = pl.du, pl.u_raw, pl.du_raw, B
            if pl.itc_world > 1:
                # data parallel: the gradients of every shard's user vectors are gathered and the module's backward runs on the global
                # batch on every rank: each rank's own rows of d u_raw then carry the terms of ALL ranks' losses (the group token is built
                # from everybody's rows), which that rank alone can send on through its encoders
                ex = self._itc_exchange(pl)
                self._coll(lambda: [ex.all_gather_packed(pl.du[g].reshape(-1), pl.du_g[g].reshape(-1)) for g in (0, 1)])
                du_in, u_raw, du_out, Bm = pl.du_g, pl.u_raw_g, pl.du_raw_g, self.itc_bs
            L.call("amid_itc_mix_bwd_f32", du_in.data_ptr(), u_raw.data_ptr(), pl.itc_gate.data_ptr(), pl.itc_z.data_ptr(),
                   pl.itc_sw.data_ptr(), self._pp("itc_d{d}.trans_nn.weight"), self._pp("itc_d{d}.trans_nn.bias"),
                   self._pp("itc_d{d}.trans_bs.weight"), Bm, D, du_out.data_ptr(), self._pp("itc_d{d}.trans_nn.weight", G),
                   self._pp("itc_d{d}.trans_nn.bias", G), self._pp("itc_d{d}.trans_bs.weight", G), self._pp("itc_d{d}.trans_bs.bias", G), s)
            if pl.itc_world > 1:
                ex = self._itc_exchange(pl)
                pl.du_raw.copy_(pl.du_raw_g[:, ex.rank * B:(ex.rank + 1) * B])
                # the module's own parameter gradients came out of the GLOBAL batch, identically on every rank: the step's dense exchange
                # sums the ranks' gradients, so each rank contributes its 1 / world share
                for d in (1, 2):
                    for name in ("trans_nn.weight", "trans_nn.bias", "trans_bs.weight", "trans_bs.bias"):
                        self.dense.view(f"itc_d{d}.{name}", G).mul_(1.0 / ex.world)
            du = pl.du_raw
        L.call("amid_lnmean_bwd_f32", pl.x[2].data_ptr(), du.data_ptr(), fp.ptr("sac1.last_layernorm.weight"),
               fp.ptr("sac2.last_layernorm.weight"), B, T, D, SASREC_LN_EPS, pl.dxbuf.data_ptr(), pl.last_part.data_ptr(), s)

    def _scorer_fwd(self, pl: SasrecPlan, head: str, items: int, p1, p2, with_loss: bool) -> None:
        shp, fp = pl.shape, self.dense
        lib().call("amid_scorer_fwd_f32", pl.u.data_ptr(), items, fp.ptr(f"{head}.fc.0.weight"), fp.ptr(f"{head}.fc.0.bias"),
                   fp.ptr(f"{head}.fc.2.weight"), fp.ptr(f"{head}.fc.2.bias"), pl.labels.data_ptr() if with_loss else None,
                   pl.domain.data_ptr() if with_loss else None, shp.B, shp.NI, self.D, self.hid, p1.data_ptr(), p2.data_ptr(),
                   pl.dp1.data_ptr() if with_loss else None, pl.dp2.data_ptr() if with_loss else None,
                   pl.loss_part.data_ptr() if with_loss else None, self.s)

    def _scorer_bwd(self, pl: SasrecPlan, head: str, items: int, ditems: int, p1, p2, dp1, dp2, part, accumulate: int) -> None:
        shp, fp = pl.shape, self.dense
        lib().call("amid_scorer_bwd_f32", pl.u.data_ptr(), items, fp.ptr(f"{head}.fc.0.weight"), fp.ptr(f"{head}.fc.0.bias"),
                   fp.ptr(f"{head}.fc.2.weight"), fp.ptr(f"{head}.fc.2.bias"), p1.data_ptr(), p2.data_ptr(), dp1.data_ptr(), dp2.data_ptr(),
                   shp.B, shp.NI, self.D, self.hid, pl.du.data_ptr(), ditems, part.data_ptr(), accumulate, self.s)

    # ---- isItC head: last LayerNorm + mean -> pair-max -> batch-softmax gate + mix -> scorer (csrc/intercomp.hip) ----
    def _enqueue_head_itc_fwd(self, pl: SasrecPlan, items: int, with_loss: bool) -> None:
        self._enqueue_user_vectors(pl)
        self._scorer_fwd(pl, "predictModule", items, pl.p1, pl.p2, with_loss)

    def _enqueue_head_itc_bwd(self, pl: SasrecPlan, items: int, ditems: int) -> None:
        self._scorer_bwd(pl, "predictModule", items, ditems, pl.p1, pl.p2, pl.dp1, pl.dp2, pl.sc_part, 0)
        self._enqueue_user_vectors_bwd(pl)

    # ---- isDR head (next-4): three scorers on the same (u, items) + the doubly-robust objective of the current mode ----
    def _enqueue_head_dr_fwd(self, pl: SasrecPlan, items: int, with_loss: bool) -> None:
        L, shp = lib(), pl.shape
        self._enqueue_user_vectors(pl)
        self._scorer_fwd(pl, "predictModule", items, pl.p1, pl.p2, False)
        self._scorer_fwd(pl, "predict_ips", items, pl.ips1, pl.ips2, False)
        self._scorer_fwd(pl, "predict_gfunc", items, pl.g1, pl.g2, False)
        if with_loss:
            pa = lambda a, b: ptr_array([a.data_ptr(), b.data_ptr()])       # noqa: E731
            L.call("amid_dr_loss_f32", pa(pl.p1, pl.p2), pa(pl.ips1, pl.ips2), pa(pl.g1, pl.g2), pl.labels.data_ptr(), pl.domain.data_ptr(),
                   pl.in_ob.data_ptr(), self.dr_mode, self.dr_e_w, shp.B, shp.NI, pa(pl.dp1, pl.dp2), pa(pl.dips1, pl.dips2),
                   pa(pl.dg1, pl.dg2), pl.dr_loss_part.data_ptr(), self.s)

    def _enqueue_head_dr_bwd(self, pl: SasrecPlan, items: int, ditems: int) -> None:
        self._scorer_bwd(pl, "predictModule", items, ditems, pl.p1, pl.p2, pl.dp1, pl.dp2, pl.sc_part, 0)
        self._scorer_bwd(pl, "predict_ips", items, ditems, pl.ips1, pl.ips2, pl.dips1, pl.dips2, pl.sc_part_ips, 1)
        self._scorer_bwd(pl, "predict_gfunc", items, ditems, pl.g1, pl.g2, pl.dg1, pl.dg2, pl.sc_part_g, 1)
        self._enqueue_user_vectors_bwd(pl)

    def _enqueue_scorers_fused(self, pl: SasrecPlan, items: int, ditems: int, tr_src, tr_dst, n_tr: int) -> None:
        """Every scorer of the model (one, or the three of isDR) forward + the row's loss terms + backward on pl.u in ONE launch
        (amid_scorer_multi_fwd_bwd_f32): pl.du, d items, per-head weight-gradient partials, loss partials."""
        shp, fp = pl.shape, self.dense
        heads = DR_HEADS if self.dr else DR_HEADS[:1]
        outs = [(pl.p1, pl.p2, pl.dp1, pl.dp2, pl.sc_part)]
        if self.dr:
            outs += [(pl.ips1, pl.ips2, pl.dips1, pl.dips2, pl.sc_part_ips), (pl.g1, pl.g2, pl.dg1, pl.dg2, pl.sc_part_g)]
        pa = lambda seq: ptr_array(list(seq))          # noqa: E731
        lib().call_named("amid_scorer_multi_fwd_bwd_f32", u=pl.u.data_ptr(), items=items, w1=pa(fp.ptr(f"{h}.fc.0.weight") for h in heads),
                         b1=pa(fp.ptr(f"{h}.fc.0.bias") for h in heads), w2=pa(fp.ptr(f"{h}.fc.2.weight") for h in heads),
                         b2=pa(fp.ptr(f"{h}.fc.2.bias") for h in heads), n_heads=len(heads), labels=pl.labels.data_ptr(), domain_id=pl.domain.data_ptr(),
                         ob_label=pl.in_ob.data_ptr() if self.dr else None, mode=self.dr_mode if self.dr else 0, dr_e_w=self.dr_e_w, B=shp.B, NI=shp.NI,
                         D=self.D, hid=self.hid, p1=pa(o[0].data_ptr() for o in outs), p2=pa(o[1].data_ptr() for o in outs),
                         dp1=pa(o[2].data_ptr() for o in outs), dp2=pa(o[3].data_ptr() for o in outs), loss_part=pl.loss_part.data_ptr(),
                         dr_loss_part=pl.dr_loss_part.data_ptr() if self.dr else None, du=pl.du.data_ptr(), ditems=ditems,
                         sc_part=pa(o[4].data_ptr() for o in outs), tr_src=tr_src, tr_dst=tr_dst, n_tr=n_tr, stream=self.s)

    # ---- listwise objectives (loss = "softmax" | "bpr"): user vectors -> amid_scorer_listwise_fwd_bwd_f32 -> their backward ----
    def _listwise_fwd(self, pl: SasrecPlan, with_loss: bool, sum_loss: bool) -> bool:
        """The forward's head under a listwise loss: the user vectors only (pl.u; InterComp's mix included).  The scorer's forward, the
        objective and the scorer's backward are ONE launch, enqueued by the backward that follows (_listwise_bwd): pl.p1 / pl.p2, the loss
        partials and -- sum_loss -- pl.loss are there after enqueue_backward.  False: not this engine's case (the BCE heads run)."""
        pl.listwise_owed = False
        if self.loss == "bce" or not with_loss:
            return False
        if getattr(pl, "itc_world", 1) != 1 or getattr(pl, "inc_world", 1) != 1:
            raise ValueError(f"loss = {self.loss!r}: the listwise step is single-GPU (a data-parallel shard of a comp batch is refused)")
        if pl.shape.NI < 2 or pl.shape.NI > 1024:
            raise ValueError(f"loss = {self.loss!r} needs 1 .. 1023 negatives a row, got {pl.shape.NI - 1}")
        if self.hard_negs and self.hard_skip + self.hard_negs > pl.shape.NI - 1:
            raise ValueError(f"hard_skip + hard_negs = {self.hard_skip} + {self.hard_negs} exceeds the {pl.shape.NI - 1} negatives of a row")
        self._enqueue_user_vectors(pl)
        pl.listwise_owed, pl.listwise_sum = True, bool(sum_loss)
        return True

    def _listwise_bwd(self, pl: SasrecPlan, items: int, ditems: int, tr_src, tr_dst, n_tr: int) -> bool:
        """The launch _listwise_fwd left to the backward (pl.dp1 / pl.dp2 then hold dLoss/dz, not dLoss/dp), and the user vectors' backward."""
        if not getattr(pl, "listwise_owed", False):
            return False
        pl.listwise_owed = False
        shp = pl.shape
        io = dict(u=pl.u.data_ptr(), items=items, domain_id=pl.domain.data_ptr(), kind=LOSSES.index(self.loss), B=shp.B, NI=shp.NI, D=self.D,
                  hid=self.hid, p1=pl.p1.data_ptr(), p2=pl.p2.data_ptr(), dz1=pl.dp1.data_ptr(), dz2=pl.dp2.data_ptr(),
                  loss_part=pl.loss_part.data_ptr(), du=pl.du.data_ptr(), ditems=ditems, sc_part=pl.sc_part.data_ptr(), tr_src=tr_src,
                  tr_dst=tr_dst, n_tr=n_tr, stream=self.s)
        if self.hard_negs:          # the mined list: pl.sel [B, H] the kept positions, pl.z [B, NI] the own domain's logits (section 18)
            lib().call_named("amid_scorer_mined_fwd_bwd_f32", self._scorer(), io, keep=self.hard_negs, skip=self.hard_skip,
                             sel=pl.sel.data_ptr(), z=pl.z.data_ptr())
        else:
            lib().call_named("amid_scorer_listwise_fwd_bwd_f32", self._scorer(), io)
        self._enqueue_user_vectors_bwd(pl)
        if pl.listwise_sum:
            lib().call("amid_sum_vector_f32", pl.loss_part.data_ptr(), shp.B, pl.loss.data_ptr(), self.s)
        return True

    def _head_io(self, pl: SasrecPlan, items: int, ditems: int):
        """What the one-launch heads (forward + loss + backward) read and write beside the parameters, under the header's names."""
        shp = pl.shape
        return dict(x=pl.x[2].data_ptr(), items=items, labels=pl.labels.data_ptr(), domain_id=pl.domain.data_ptr(), B=shp.B, T=shp.Tenc, NI=shp.NI,
                    D=self.D, hid=self.hid, eps=SASREC_LN_EPS, u=pl.u.data_ptr(), p1=pl.p1.data_ptr(), p2=pl.p2.data_ptr(), dp1=pl.dp1.data_ptr(),
                    dp2=pl.dp2.data_ptr(), loss_part=pl.loss_part.data_ptr(), dx=pl.dxbuf.data_ptr(), ditems=ditems,
                    ln_part=pl.last_part.data_ptr(), stream=self.s)

    def enqueue_backward(self, pl: SasrecPlan, train: bool) -> None:
        """Backward from pl.dp1 / pl.dp2 (dLoss/dp) to pl.uniq_grad (table rows) and dense.grad."""
        L, s, shp, D = lib(), self.s, pl.shape, self.D
        B, T, NI, M = shp.B, shp.Tenc, shp.NI, shp.M
        st = self.step_state.data_ptr()
        tr = 1 if train else 0
        tr_src, tr_dst, n_tr = self._wT_lists()      # transposed weights: in_proj q/k/v blocks, out_proj, conv1, conv2 for both layers and domains
        # compute = "bf16" on the strip path: the strip backward's data-gradient products take bf16 fragment images of the transposed weights
        # (the fp32 transposes are still refreshed: the row-tile fallbacks and tests read them)
        self._bf16_bwd = bool(self._ceff() == "bf16" and pl.strip)
        # (the fused per-sequence backward -- amid_sas_seq_bwd_f32 -- keeps the fp32 matrix instructions)
        self._p3_bwd = self._p3_bwd_for(pl)
        bf = 3 if self._p3_bwd else 1 if self._bf16_bwd else 0
        if self._bf16_as_f32 and self._p3_bwd:
            bf = 1                      # one bf16 piece: the strips' rings stream the hi plane of the three-plane images
        if self._bf16_bwd:
            if not hasattr(self, "wT16"):
                self.wT16 = torch.empty(2, 2, 6, D * D, dtype=torch.bfloat16, device=self.device)
            L.call("amid_sas_weights_bf16", tr_src, n_tr, D, 1, self.wT16.data_ptr(), s)
        if self._p3_bwd:
            if not getattr(pl, "wT16x3_written", False):           # (the train step's gather K1 wrote them with extra workgroups)
                L.call("amid_sas_weights_bf16_planes", tr_src, n_tr, D, 1, 3, self._wT16x3_buf().data_ptr(), s)
            pl.wT16x3_written = False
        items = pl.xg.data_ptr() + 4 * 2 * shp.Mi * D
        ditems = pl.dxg.data_ptr() + 4 * 2 * shp.Mi * D
        if self._listwise_bwd(pl, items, ditems, tr_src, tr_dst, n_tr):
            pass
        elif (self.dr or self.itc_bs) and getattr(self, "_fuse_scorers", False):
            self._enqueue_scorers_fused(pl, items, ditems, tr_src, tr_dst, n_tr)
            self._enqueue_user_vectors_bwd(pl)
        elif self.dr:
            L.call("amid_transpose_weights_f32", tr_src, tr_dst, n_tr, D, s)
            self._enqueue_head_dr_bwd(pl, items, ditems)
        elif self.itc_bs:
            L.call("amid_transpose_weights_f32", tr_src, tr_dst, n_tr, D, s)
            self._enqueue_head_itc_bwd(pl, items, ditems)
        elif getattr(pl, "head_done", False):
            pl.head_done = False          # (the forward's workgroups ran the head: amid_sas_seq_fwd_split_lnstat_head_f32 in enqueue_forward)
        elif getattr(self, "_fuse_head", False) and getattr(pl, "tail2", False) and getattr(self, "_live_fwd", False) and self._live_list(pl) is not None:
            # the folded step: the scorer's weight gradients leave the head as per-sample hidden gradients (pl.hidg; the gradient tail sums
            # them, amid_grad_tail_live_f32) and the fp32 transposes are not refreshed (this step's strips read the three-plane images)
            L.call_named("amid_head_fwd_bwd_own_vec_f32", self._last_ln(), self._scorer(), self._head_io(pl, items, ditems),
                         hidg=self._hidg(pl).data_ptr(), tr_src=None, tr_dst=None, n_tr=0)
        elif getattr(self, "_fuse_head", False):
            L.call_named("amid_head_fwd_bwd_own_f32" if getattr(self, "_live_fwd", False) and self._live_list(pl) is not None else "amid_head_fwd_bwd_f32",
                         self._last_ln(), self._scorer(), self._head_io(pl, items, ditems), sc_part=pl.sc_part.data_ptr(), tr_src=tr_src,
                         tr_dst=tr_dst, n_tr=n_tr)
        else:
            L.call_named("amid_head_bwd_f32", self._last_ln(), self._scorer(), x=pl.x[2].data_ptr(), u=pl.u.data_ptr(), items=items,
                         p1=pl.p1.data_ptr(), p2=pl.p2.data_ptr(), dp1=pl.dp1.data_ptr(), dp2=pl.dp2.data_ptr(), B=B, T=T, NI=NI, D=D,
                         hid=self.hid, eps=SASREC_LN_EPS, dx=pl.dxbuf.data_ptr(), ditems=ditems, ln_part=pl.last_part.data_ptr(),
                         sc_part=pl.sc_part.data_ptr(), tr_src=tr_src, tr_dst=tr_dst, n_tr=n_tr, stream=s)
        drop = dict(tmq=pl.tmq.data_ptr(), step_state=st, train=tr, p_drop=SASREC_P_DROP)

        lv = self._live_list(pl)
        live_attn = lv is not None and bool(lib().value("amid_attn_live_supported", T, D, self.H, 1))
        att = dict(d_o=pl.d_o.data_ptr(), B=B, T=T, D=D, H=self.H, causal=1, step_state=st, train=tr, p_drop=SASREC_P_DROP, stream=s)

        def attn_bwd(l):
            if live_attn:        # the live sequences only; the others' rows of dq / dk / dv are never read (strip kernels, wgrad hint)
                L.call_named("amid_attn_bwd_live_f32", self._saved(pl, l), self._grads(pl, l), att, layer=l, live=lv)
                return
            L.call_named("amid_attn_bwd_rows_f32", self._saved(pl, l), self._grads(pl, l), att, layer=l, key_keep=None, row_domain=self._own_rows(pl))

        # live: the three row-tile kernels walk the sequences that carry a gradient only (see _own_rows), re-tiled over the CUs
        dom = self._own_rows(pl)
        live = dom is not None and pl.live_rows
        dx_in = (pl.dx0 if self.inc_bs else pl.dxg).data_ptr()
        seq = bool(pl.strip and lv is not None and live and live_attn and self._seq_backward(pl))
        pl.seq_bwd_used = seq              # (what THIS backward ran: _seq_backward() depends on the step being enqueued; bench.py and tests read this)
        if seq:
            # the five launches below as one workgroup-long chain per live sequence
            sv = self._seq_ptrs(pl)
            L.call_named("amid_sas_seq_bwd_f32", sv, self._seq_grad_ptrs(pl), self._fams(), self._wT_fams(bf), n_layers=2, dxo=pl.dxbuf.data_ptr(),
                         tmq=pl.tmq.data_ptr(), x=sv["x_in"], ln_eps=SASREC_LN_EPS, B=B, T=T, D=D, H=self.H, live=lv, step_state=st, train=tr,
                         p_drop=SASREC_P_DROP, d_o=pl.d_o.data_ptr(), dx=dx_in, mma_bf16=bf, stream=s)
        elif pl.strip:
            # a train step's index sort rides in these three launches (phases 2, 3, 4; phase 1 rode in the catch-up launch)
            riding = getattr(pl, "riding", False)
            sfx = "_sort" if riding else ""
            t2 = getattr(pl, "tail2", False)
            plan_addr = (self._sort_plan_c(pl) if t2 else self._sort_plan(pl)) if riding else None
            ride = lambda ph: dict(sort_plan=plan_addr, sort_phase=ph) if riding else {}      # noqa: E731
            strip = dict(ln_eps=SASREC_LN_EPS, B=B, T=T, D=D, live=lv, stream=s)
            L.call_named(f"amid_sas_strip_ffn_bwd{sfx}_f32", self._ffn_bwd_block(pl, 1, False), strip, drop, ride(2), dxo=pl.dxbuf.data_ptr(),
                         mma_bf16=self._strip_mode(bf, 0))
            attn_bwd(1)
            # layer 1's q / k / v + LayerNorm1 backward and layer 0's feed-forward / out-projection backward: one launch
            fused = (self._qkv_bwd_block(pl, 1, False), self._ffn_bwd_block(pl, 0, False, fused=True), strip, drop, ride(3))
            if t2:      # ... whose idle CUs also sum the scorer's weight gradients from the head's per-sample hidden gradients
                # (a prepared pool: the same launch without the sort's workgroups)
                L.call_named(f"amid_sas_strip_qkv_bwd{sfx}_scorer_f32", *fused, self._scorer(("dW1", "db1", "dW2", "db2"), grad=True),
                             mma_bf16=self._strip_mode(bf, 1), hidg=self._hidg(pl).data_ptr(), u=pl.u.data_ptr(), items=items, NI=NI, hid=self.hid)
            else:
                L.call_named(f"amid_sas_strip_qkv_bwd{sfx}_f32", *fused, dx=None, mma_bf16=self._strip_mode(bf, 1))
            attn_bwd(0)
            if t2:      # ... with the embedding layer's backward applied on the strip (no amid_embed_bwd launch)
                L.call_named("amid_sas_strip_qkv_bwd_emb_f32", self._qkv_bwd_block(pl, 0, False), strip, ride(4) if riding else NO_SORT_RIDERS, dx=dx_in,
                             emb_tmq=pl.tmq.data_ptr(), step_state=st, train=tr, emb_p_drop=SASREC_P_DROP, mma_bf16=self._strip_mode(bf, 2))
            else:
                L.call_named(f"amid_sas_strip_qkv_bwd{sfx}_f32", self._qkv_bwd_block(pl, 0, False), NO_FUSED_FFN, strip, ride(4), dx=dx_in,
                             mma_bf16=self._strip_mode(bf, 2))
        else:
            rows, suf, rpt = ("_rows", pl.rt_suffix_v, pl.rpt_v) if live else ("", pl.rt_suffix, pl.rpt)
            hint = dict(row_domain=dom, B=B, T=T) if live else {}
            tile = dict(ln_eps=SASREC_LN_EPS, M=M, D=D, rows_per_tile=rpt, mma_bf16=self.mma_bf16, stream=s)
            L.call_named(f"amid_sas_ffn_bwd{rows}_f32" + suf, self._ffn_bwd_block(pl, 1, live), tile, drop, hint, dxo=pl.dxbuf.data_ptr())
            attn_bwd(1)
            # layer 1's q / k / v + LayerNorm1 backward and layer 0's feed-forward / out-projection backward: one launch
            L.call_named(f"amid_sas_qkv_ffn_bwd{rows}_f32" + suf, self._qkv_bwd_block(pl, 1, live), self._ffn_bwd_block(pl, 0, live, fused=True), tile, drop, hint,
                         dx=pl.dxbuf.data_ptr())
            attn_bwd(0)
            L.call_named(f"amid_sas_qkv_bwd{rows}_f32" + suf, self._qkv_bwd_block(pl, 0, live), tile, hint, dx=dx_in)
        dy, xx = [], []
        for l in (0, 1):
            dy += [pl.dq_l[l].data_ptr(), pl.dk_l[l].data_ptr(), pl.dv_l[l].data_ptr(), pl.dr[l].data_ptr(), pl.dpre1[l].data_ptr(),
                   pl.dpre2[l].data_ptr()]
            xx += [pl.qn[l].data_ptr(), pl.x[l].data_ptr(), pl.x[l].data_ptr(), pl.o[l].data_ptr(), pl.y[l].data_ptr(), pl.h[l].data_ptr()]
        # NOTE: pl.x[0] is the gathered-row buffer xg, still intact here (its gradient lives in dxg)
        wgrad = lambda: dict(self._on_plan(pl, "wgrad_tab", lambda: dict(      # noqa: E731  (dy, x: read when the launch is enqueued)
            n_layers=2, M=M, D=D, splits=pl.splits, w_part=ptr_array([pl.w_part[0].data_ptr(), pl.w_part[1].data_ptr()]),
            b_part=ptr_array([pl.b_part[0].data_ptr(), pl.b_part[1].data_ptr()]), B=B, T=T)), dy=ptr_array(dy), x=ptr_array(xx),
            row_domain=self._own_rows(pl), stream=s)
        t2 = bool(getattr(pl, "tail2", False) and pl.strip and not seq)
        if t2:      # the last phase of the step's index sort (run heads) rides in the weight gradients; the embedding backward is done
            if getattr(pl, "lnstat_fwd", False):      # the forward stored row statistics instead of qn / y: the operands of q's and conv1's
                for l in (0, 1):                       # gradients are rebuilt from x / r while they are staged
                    xx[6 * l + 0], xx[6 * l + 4] = pl.x[l].data_ptr(), pl.r[l].data_ptr()
                self._wgrad_one = True              # (the folded bf16 step: this launch on ONE piece per operand, _wgrad_mode -> 4)
                try:
                    wmode = self._wgrad_mode(D)
                finally:
                    self._wgrad_one = False
                # (of the families it takes the four LayerNorm ones; a prepared pool: no rider z-slice)
                L.call_named("amid_sas_wgrad_rows_sort_ln_f32" if pl.riding else "amid_sas_wgrad_rows_ln_f32", self._fams(), wgrad(),
                             dict(sort_plan=self._sort_plan_c(pl)) if pl.riding else {}, mma_bf16=wmode, ln_stat=self._ln_stat(pl)[1])
            elif not pl.riding:
                L.call_named("amid_sas_wgrad_rows_f32", wgrad(), mma_bf16=self._wgrad_mode(D))
            else:
                L.call_named("amid_sas_wgrad_rows_sort_f32", wgrad(), mma_bf16=self._wgrad_mode(D), sort_plan=self._sort_plan_c(pl))
            self._enqueue_grad_tail(pl, live, seq)
            return
        L.call_named("amid_sas_wgrad_rows_f32", wgrad(), mma_bf16=self._wgrad_mode(D))
        emb = dict(dxg=dx_in, tmq=pl.tmq.data_ptr(), B=B, T=T, D=D, nsplit=pl.pos_splits, dpos_part=pl.dpos_part.data_ptr(), step_state=st,
                   train=tr, p_drop=SASREC_P_DROP, stream=s)
        if getattr(pl, "riding", False):     # the last phase of the step's index sort (run heads) rides here
            L.call_named("amid_embed_bwd_sort_f32", emb, row_domain=dom if live else None, sort_plan=self._sort_plan(pl), sort_phase=5)
        elif live:     # the dead sequences' rows of the encoder-input gradient were never written: zero-filled here, not read
            L.call_named("amid_embed_bwd_rows_f32", emb, row_domain=dom)
        else:
            L.call_named("amid_embed_bwd_f32", emb)
        if self.inc_bs:      # InnerComp's parameter gradients; the rows' own halves + its share -> the table-row gradient buffer
            G = self.dense.grad
            head = (pl.dpos_part.data_ptr(), pl.pos_splits, pl.xg.data_ptr(), pl.dx0.data_ptr(), pl.inc_gate.data_ptr(), pl.inc_S.data_ptr(),
                    pl.inc_sw.data_ptr(), self._pp("inc_d{d}.trans_nn.weight"), self._pp("inc_d{d}.trans_nn.bias"),
                    self._pp("inc_d{d}.trans_bs.weight"), B, shp.T, D)
            outs = (pl.inc_dZ.data_ptr(), pl.inc_dS.data_ptr(), pl.inc_rows.data_ptr(), self._pp("inc_d{d}.trans_nn.weight", G),
                    self._pp("inc_d{d}.trans_nn.bias", G), self._pp("inc_d{d}.trans_bs.weight", G), self._pp("inc_d{d}.trans_bs.bias", G),
                    pl.dxg.data_ptr(), s)
            if getattr(pl, "inc_world", 1) > 1:
                # data parallel: the token group is shared by the GLOBAL batch, so its gradient dZ is the sum of every rank's pos_emb
                # partials of rows T .. 2T - 1: all-reduced between the two phases.  W_nn / b_nn / b_bs gradients then come out alike on
                # every rank (1 / world each: the dense exchange sums the ranks); trans_bs.weight's gradient is this rank's slice
                ex = self._inc_exchange(pl)
                shard = (self.inc_bs, ex.rank * B)
                L.call("amid_inc_bwd_shard_f32", *head, *shard, 1, 1.0 / ex.world, *outs)
                self._coll(lambda: ex.all_reduce_dense(pl.inc_dZ))
                L.call("amid_inc_bwd_shard_f32", *head, *shard, 2, 1.0 / ex.world, *outs)
            else:
                L.call("amid_inc_bwd_f32", *head, *outs)
        self._enqueue_grad_tail(pl, live, seq)

    def _enqueue_grad_tail(self, pl: SasrecPlan, live: bool = False, seq: bool = False) -> None:
        """The two independent, bandwidth-bound ends of backward side by side in one launch: the fixed-order sum of every partial
        buffer (dense gradients + loss) and the segment reduce of the table-row gradients."""
        L, s, shp = lib(), self.s, pl.shape
        if getattr(self, "_sort_owed", False):    # no fork point of this engine's backward launched the deferred sort: do it now
            self.ev_idx.record(self.stream)
            self.enqueue_sort(pl)
        self.join_sort()                          # pos_sorted / seg_off come from the side-stream sort
        blk = (pl.red_blk_s if seq else getattr(pl, "red_blk_v", None) if live else None) or pl.red_blk   # per-entry block ranges of the partial sums
        ent, n_ent, ent_max = ((pl.red_entries_s, pl.red_n_s, pl.red_max_s) if seq else (pl.red_entries_v, pl.red_n_v, pl.red_max_v) if live
                               else (pl.red_entries, pl.red_n, pl.red_max))
        pk = getattr(self, "_tail_pack", None)
        pl.spans_done = False
        seg = self._seg(pl)
        if pk is not None:       # graph A of the data-parallel step: the reduced rows go into this rank's exchange chunk, packed by the tail
            seg = dict(seg, **self._pack_block(pl, pk))
        red = lambda e, n, b: dict(entries_dev=e.data_ptr(), n_entries=n, blk_off=b[0].data_ptr(), total_blocks=b[1])      # noqa: E731
        pos_rows = lambda: dict(self._dpos(), live=pl.live.data_ptr(), B=shp.B, T=shp.Tenc)      # noqa: E731  (the folded tails sum the position rows' gradients)
        if getattr(pl, "tail2", False) and not getattr(self, "_in_train_step", False):
            # the folded step under data parallel: the exchange ships finished rows, so phase B of the segment reduce is a launch of its own
            # behind the tail -- and in graph A of the graph pair the packing of this rank's chunk (ids | rows | dense) rides in it
            fp = self.dense
            tail = (red(*self._tail2_table(pl)), pos_rows(), dict(n_idx=pl.n_compact, D=self.D, stream=s))
            if self.FUSED_OPT:        # ... all of it as ONE launch (amid_grad_tail_opt_f32's workgroups, shipping instead of applying)
                left_lo = fp.slots["predictModule.fc.0.weight"][0]      # the scorer's gradients: final before this launch (the strip riders)
                dense = (self._adam_dense(), self._uniq(pl), dict(left_lo=left_lo, left_hi=fp.numel, n_uniq_max=pl.n_compact,
                                                                  ticket=pl.tail_ticket.data_ptr()))
                if pk is not None:
                    L.call_named("amid_grad_tail_live_dp1_f32", seg, *tail, *dense)
                else:
                    L.call_named("amid_grad_tail_live_dp1_f32", seg, NO_PACK, *tail, *dense)
            elif pk is not None:
                L.call_named("amid_grad_tail_live_dp_f32", seg, self._uniq(pl), *tail)
            else:
                L.call_named("amid_grad_tail_live_dp_f32", seg, NO_PACK, NO_UNIQ, *tail)
            pl.spans_done = True
            return
        pl.opt_done = False
        opt = dict(grad_scale=self.grad_scale, step_state=self.step_state.data_ptr(), ticket=pl.tail_ticket.data_ptr(), D=self.D, stream=s)
        if getattr(pl, "tail2", False) and self.FUSED_OPT and self.table_m is not None and not self.dr:
            # the folded step's tail AND its optimizer as one launch (round 6): every producer of a gradient slice applies Adam on the spot
            fp = self.dense
            left_lo = fp.slots["predictModule.fc.0.weight"][0]          # the scorer's slots (the flat buffer's tail): summed by the strip riders
            L.call_named("amid_grad_tail_opt_f32", seg, red(*self._tail2_table(pl)), pos_rows(), self._adam_dense(), self._adam_rows(), self._uniq(pl),
                         opt, n_idx=pl.n_compact, left_lo=left_lo, left_hi=fp.numel, n_uniq_max=pl.n_compact)
            pl.opt_done = True
            return
        if getattr(pl, "tail2", False):
            L.call_named("amid_grad_tail_live_f32", seg, red(*self._tail2_table(pl)), pos_rows(), NO_SCORER_SUMS,      # (the scorer sums rode in the
                         n_idx=pl.n_compact, D=self.D, stream=s)                                                     # middle strip launch)
            return
        if pk is not None:       # graph A of the data-parallel step: the tail also packs this rank's exchange chunk (ids | rows | dense)
            L.call_named("amid_grad_tail_pack_f32", seg, red(ent, n_ent, blk), self._uniq(pl), max_count=ent_max, n_idx=self.n_sparse(pl), D=self.D,
                         stream=s)
            return
        # a single-GPU train step's optimizer launch follows: it finishes the runs that cross chunks itself (amid_optimizer_step_spans_f32;
        # the same additions in the same order as the spans launch this saves).  Not for enqueue_local_grads: the exchange ships uniq_grad
        spans_later = bool(self.FUSED_SPANS and getattr(self, "_in_train_step", False) and self.D in (64, 128, 256))
        left = getattr(pl, "red_left_s" if seq else "red_left_v" if (live and hasattr(pl, "red_left_v")) else "red_left", None)
        if spans_later and self.FUSED_OPT and self.table_m is not None and left is not None:
            # ... and the optimizer itself: the tail's workgroups apply Adam to every slice they finish (amid_grad_tail_opt_f32 without its
            # position-row role: here every dense gradient is an entry of the reduce table) -- one launch fewer in every single-GPU step
            left_lo, left_hi = left or (0, 0)
            L.call_named("amid_grad_tail_opt_f32", seg, red(ent, n_ent, blk), NO_POS_ROWS, self._adam_dense(), self._adam_rows(), self._uniq(pl),
                         opt, n_idx=self.n_sparse(pl), left_lo=left_lo, left_hi=left_hi, n_uniq_max=self.n_sparse(pl))
            pl.opt_done = True
            return
        pl.spans_owed = self.n_sparse(pl) if spans_later else 0
        L.call_named("amid_grad_tail_nospans_f32" if spans_later else "amid_grad_tail_f32", seg, red(ent, n_ent, blk), max_count=ent_max,
                     n_idx=self.n_sparse(pl), D=self.D, stream=s)

    def _pack_block(self, pl: SasrecPlan, pk):
        """The packing a gradient tail does for graph A of the data-parallel step, from _tail_pack = (this rank's chunk, its bound, whether
        the dense gradient travels in it): the chunk is ids | rows | dense, so the REDUCED ROWS (uniq_grad) land behind its ids."""
        from .dist import packed_rows
        send, umax, with_dense = pk
        id_rows, rows = packed_rows(umax, self.D)
        return dict(uniq_grad=send.data_ptr() + 4 * id_rows * self.D, n_out=umax, pad_id=self.n_rows, out_ids=send.data_ptr(),
                    dense_src=self.dense.grad.data_ptr() if with_dense else None,
                    dense_dst=send.data_ptr() + 4 * rows * self.D if with_dense else None, dense_n=self.dense.numel if with_dense else 0,
                    err_flag=pl.err.data_ptr())

    def enqueue_optimizer(self, pl: SasrecPlan, sparse=None) -> None:
        """Dense Adam on the flat buffer + lazy row Adam on (uniq_ids, uniq_grad, n_uniq); `sparse`
        overrides the plan's local lists with the world-merged ones under data parallelism."""
        L, s = lib(), self.s
        self._ensure_opt_state()
        if sparse is None:
            lists, cap = (self._uniq(pl), self._seg(pl)), self.n_sparse(pl)
        else:
            ids, rows, nu = sparse
            lists, cap = (dict(uniq_ids=ids.data_ptr(), n_uniq=nu.data_ptr(), uniq_grad=rows.data_ptr()),), ids.numel()
        if getattr(pl, "opt_done", False):          # the gradient tail applied the step (amid_grad_tail_opt_f32)
            pl.opt_done = False
            if sparse is not None:
                raise RuntimeError("the gradient tail already applied this step's local gradients")
            return
        owed = int(getattr(pl, "spans_owed", 0))
        pl.spans_owed = 0
        t2 = getattr(pl, "tail2", False) and not getattr(pl, "spans_done", False)
        adam = (self._adam_dense(), self._adam_rows(), dict(n_uniq_max=cap, D=self.D, grad_scale=self.grad_scale,
                                                            step_state=self.step_state.data_ptr(), stream=s))
        if sparse is None and (t2 or owed):      # the segment reduce's runs across chunks are finished (and applied) here
            L.call_named("amid_optimizer_step_spans_f32", *adam, *lists, n_sorted=pl.n_compact if t2 else owed)
            return
        if owed:
            raise RuntimeError("the gradient tail left the chunk-crossing runs to an optimizer launch that takes merged lists")
        L.call_named("amid_optimizer_step_f32", *adam, *lists)

    def enqueue_loop_optimizer(self, pl: SasrecPlan, g: torch.Tensor, sqnorm: Optional[torch.Tensor] = None, max_norm: float = float("inf")) -> None:
        """The optimizer launch of the reference's own loop (amid_amd/optim.py): enqueue_optimizer's plain form reading the dense gradient
        from `g` (a flat buffer laid out like self.dense.grad: the parameters' .grad tensors are its views) instead of the engine's own;
        sqnorm (device scalar, enqueue_grad_sqnorm) + max_norm: the gradients clipped on the way (amid_optimizer_step_clip_f32)."""
        self._ensure_opt_state()
        if getattr(pl, "opt_done", False) or int(getattr(pl, "spans_owed", 0)):
            raise RuntimeError("the plan's last backward was a fused train step's: its gradients are applied already")
        adam = (self._adam_dense(g), self._adam_rows(), self._uniq(pl), self._seg(pl),
                dict(n_uniq_max=self.n_sparse(pl), D=self.D, grad_scale=self.grad_scale, step_state=self.step_state.data_ptr(), stream=self.s))
        if sqnorm is None:
            lib().call_named("amid_optimizer_step_f32", *adam)
        else:
            lib().call_named("amid_optimizer_step_clip_f32", *adam, sqnorm=sqnorm.data_ptr(), max_norm=float(max_norm))

    def enqueue_grad_sqnorm(self, pl: SasrecPlan, g: torch.Tensor, out: torch.Tensor) -> None:
        """out[0] = the squared 2-norm of the whole model's gradient: the flat dense gradient `g` and the plan's unique table rows."""
        ws = getattr(self, "_sqnorm_ws", None)
        if ws is None:
            ws = self._sqnorm_ws = torch.empty(lib().value("amid_grad_sqnorm_workspace_bytes"), dtype=torch.uint8, device=self.device)
        lib().call("amid_grad_sqnorm_f32", g.data_ptr(), self.dense.numel, pl.uniq_grad.data_ptr(), pl.n_uniq.data_ptr(), self.n_sparse(pl),
                   self.D, ws.data_ptr(), out.data_ptr(), self.s)

    def enqueue_step_begin(self) -> None:
        lib().call("amid_step_begin", self.step_state.data_ptr(), self.s)
        self.step += 1

    def enqueue_train_step(self, pl: SasrecPlan) -> None:
        """Whole step t on the current stream: t += 1; unique; catch-up; forward; loss; backward; Adam."""
        self._in_train_step = True
        try:
            self.enqueue_prepare(pl, sparse=True, bump_step=True, defer_sort=True)
            self.enqueue_catchup(pl)
            self._fork_sort(pl)
            self._enqueue_fwd_bwd(pl)
            self.enqueue_optimizer(pl)
        finally:
            self._in_train_step = False
            self._bf16_as_f32 = False

    # ------------------------------------------------------------------ data parallel (one process per GPU)
    def enqueue_local_grads(self, pl: SasrecPlan) -> None:
        """Everything of step t that needs no communication: t += 1 .. local segment-reduced gradients."""
        self._in_local_grads = True
        try:
            self.enqueue_prepare(pl, sparse=True, bump_step=True, defer_sort=True)
            self.enqueue_catchup(pl)
            self._fork_sort(pl)
            self._enqueue_fwd_bwd(pl)
        finally:
            self._in_local_grads = False
            self._bf16_as_f32 = False

    def _fork_sort(self, pl: SasrecPlan) -> None:
        """Start the side-stream sort behind the catch-up launch, beside the forward (forks behind the forward or beside the weight
        gradients were measured and lost: DESIGN.md section 5)."""
        if getattr(pl, "compact", False) or getattr(pl, "fold_catchup", False):
            return                                    # the compact index list is K1's by-product / no catch-up launch: the fork follows K1
        if getattr(self, "_sort_owed", False):
            self.enqueue_sort(pl)

    FUSED_HEAD = True          # the plain SASRec head (no isItC / isDR) can run forward + backward as one launch
    HEAD_ON_FWD = True         # the folded step's head on the tail of the forward's workgroups (one launch fewer: eleven)
    HEAD_ON_FWD_KEEPS_X = False   # (tests: the last layer's output is stored all the same)

    def _enqueue_fwd_bwd(self, pl: SasrecPlan) -> None:
        """Forward (loss included; its sum rides in the gradient tail) + backward of a training step."""
        self._fuse_head = self.FUSED_HEAD and not self.dr and not self.itc_bs and self.loss == "bce"
        self._fuse_scorers = self.FUSED_HEAD and bool(self.dr or self.itc_bs) and (not self.dr or pl.shape.NI <= 16)
        # the step's own loss masks row b's terms of domain 1 - domain_id[b] with zero (train_sr.py:205-211; the doubly-robust
        # objectives likewise, train_sr_dr.py:216-221, :392-394): the encoder of that domain gets an all-zero gradient for row b.
        # InterComp AFTER the encoders mixes the rows' user vectors, so every sequence has a gradient there.
        self._own_domain_only = not self.itc_bs
        # ... and neither do the other domain's logits of a sample: with the plain head (no isDR heads, no InterComp / InnerComp) and
        # the matrix-core attention kernels the forward encodes the B live sequences only.  model.forward, which RETURNS both
        # domains' logits (model_seq.py:442), keeps encoding everything.
        self._live_fwd = self._own_domain_only and self._fuse_head and self.live_forward_ok(pl)
        try:
            self.enqueue_forward(pl, train=True, with_loss=True, sum_loss=False)
            self.enqueue_backward(pl, train=True)
        finally:
            self._fuse_head = self._fuse_scorers = self._own_domain_only = self._live_fwd = False

    LIVE_FORWARD = True        # the fused train step may skip the forward of the sequences its loss never reads
    SEQ_FORWARD = True         # the encoder forward as one launch per step where csrc/sasrec_seq.hip covers the shape

    def _live_list(self, pl: SasrecPlan):
        """Device pointer of the plan's live-sequence list (filled by amid_live_list_i32 at the head of enqueue_forward) when the
        step's loss masks the other domain of every sample and the encoder runs on the strip kernels, else None."""
        return pl.live.data_ptr() if getattr(self, "_own_domain_only", False) and pl.strip else None

    def _own_rows(self, pl: SasrecPlan):
        """Device pointer of the batch's domain ids when backward may treat the other domain's sequences as gradient-free (see
        _enqueue_fwd_bwd), else None: a backward driven by someone else's loss (the autograd path) makes no such promise."""
        return pl.domain.data_ptr() if getattr(self, "_own_domain_only", False) else None

    # ------------------------------------------------------------------ evaluation: test(), train_sr.py:31-128
    # The evaluation batch in three launches (round 6; four while K1 is its own launch, GATHER_ON_FWD = False): index marshal + live list, K1 over the live sequences only (no candidate rows: the
    # head gathers them), the inference forward over the live sequences (nothing saved), amid_eval_head_f32 (LN_last + mean, the scorer over
    # the 1 + neg_nums candidates, masked BCE, the positive's rank).  test() reads only the own domain's logits of a sample (utils.py:21-40)
    # and masks the other domain's loss terms (train_sr.py:63-64), so nothing else is computed; model.forward keeps returning both.
    # The isDR / isItC / isInC models (one GPU, the whole bs-row batch in the plan) keep the launches their forward forms the user vectors
    # with -- the bits of enqueue_forward(train=False) -- and gain the head: no [B, NI, D] copy of the candidates' rows, BCE and ranks in the
    # scorer's launch, one graph replay a batch.
    #   isDR:   the plain model's marshal + forward over the live sequences, amid_lnmean_fwd_f32 (this model's LN_last + mean: its own
    #           kernel, compiled apart from the fused head's, so its vector is READ), amid_eval_head_u_f32.  predict_ips / predict_gfunc
    #           are not evaluated: test() reads outs[0], outs[1] only.
    #   isItC:  marshal, K1 over BOTH domains' sequences (the group token is built from every row's other-domain features), the inference
    #           forward with a null live list, amid_itc_pairmax_f32 (s, u_raw), amid_eval_head_u_f32 with the mix as its prologue (32 .. 256
    #           rows, D 64 / 128: five launches; other batches: amid_itc_mix_fwd_f32 in front of it, the head reading pl.u).
    #   isInC:  marshal + enqueue_forward's own gather / token group / encoder launches over the 2T-token rows (gather_items=False,
    #           head=False), then amid_eval_head_f32 on pl.x[2] (+ isDR: amid_lnmean_fwd_f32 and amid_eval_head_u_f32).
    #   beyond 64 tokens (plain, isDR, isItC; fp32, D 128, 64 < T <= 256: _eval_long): the one-launch forward does not reach there, so the
    #           encoder is seven launches on the strip kernels' inference forms -- marshal, layer 0's q / k / v gathering its own rows (no K1),
    #           the long attention core over the live list, out-projection / feed-forward + layer 1's q / k / v, attention, out-projection /
    #           feed-forward, the head -- each the arithmetic enqueue_forward(train=False) runs for the shape, over the live rows only.
    EVAL_FUSED = True
    EVAL_LONG = True           # ... also at 64 < T <= 256 (False: those shapes evaluate through enqueue_forward, as before)

    def _eval_long(self, pl: SasrecPlan) -> bool:
        """Whether the evaluation batch's encoders are the strip launches' inference forms around the long attention core's live form."""
        shp, L = pl.shape, lib()
        return bool(self.EVAL_LONG and pl.strip and self.compute == "f32" and self._ceff() != "bf16" and self.D == 128 and not self.inc_bs
                    and L.value("amid_attn_long_live_supported", shp.Tenc, self.D, self.H) and L.value("amid_sas_strip_infer_supported", shp.Tenc, self.D))

    def eval_fused_ok(self, pl: SasrecPlan) -> bool:
        shp = pl.shape
        if not self.EVAL_FUSED or getattr(self, "comp", "") or self.input_pool(pl) is not None:
            return False
        if getattr(pl, "itc_world", 1) != 1 or getattr(pl, "inc_world", 1) != 1:      # a data-parallel shard of a comp batch keeps enqueue_forward
            return False
        if self.inc_bs:          # the encoders are enqueue_forward's for any shape; the head's own limits (amid_eval_head_f32)
            return bool(self.D % 32 == 0 and self.D <= 128 and 0 < self.hid <= 64 and self.hid % 4 == 0)
        return bool((pl.strip and self.SEQ_FORWARD and lib().value("amid_sas_seq_supported", shp.B, shp.Tenc, self.D, self.H)) or self._eval_long(pl))

    def _eval_out(self, pl: SasrecPlan):
        """The batch's results, one int32 image [rank B | rank_raw B | loss_part B (fp32 bits)] (+ the scores, for tests)."""
        if not hasattr(pl, "ev_out"):
            B = pl.shape.B
            pl.ev_out = torch.zeros(3 * B, dtype=torch.int32, device=self.device)
            pl.ev_rank, pl.ev_rank_raw, pl.ev_loss_part = pl.ev_out[:B], pl.ev_out[B:2 * B], pl.ev_out[2 * B:].view(torch.float32)
            pl.ev_p = torch.zeros(B, pl.shape.NI, dtype=torch.float32, device=self.device)
            pl.ev_u = torch.zeros(B, self.D, dtype=torch.float32, device=self.device)
            torch.cuda.synchronize(self.device)
        return pl.ev_out

    def enqueue_eval(self, pl: SasrecPlan, fix_value: float, with_loss: bool = True, want_scores: bool = False, build_images: bool = True) -> None:
        """One test() batch from the plan's static inputs (load_batch / load_packed) to pl.ev_rank / ev_rank_raw / ev_loss_part.
        build_images=False: the forward's weight images are current (eval_epoch builds them once for all its batches: the weights do not
        change inside an evaluation)."""
        if not self.eval_fused_ok(pl):
            raise ValueError("enqueue_eval: this model / shape evaluates through enqueue_forward (eval_fused_ok)")
        L, s, shp, D = lib(), self.s, pl.shape, self.D
        B, T, NI = shp.B, shp.Tenc, shp.NI
        self._eval_out(pl)
        L.call_named("amid_pack_indices_live", self._marshal(pl), step_state=None, stream=s)
        if self._eval_through_forward():           # enqueue_forward's launches up to the last encoder layer, the sequences' rows only
            self.enqueue_forward(pl, train=False, with_loss=False, head=False, gather_items=False)
        else:
            self._enqueue_eval_encoders(pl, build_images)
        ids = pl.idx_all.data_ptr() + 4 * 2 * shp.Mi
        head = dict(table=self.table.data_ptr(), ids=ids, labels=pl.labels.data_ptr() if with_loss else None, domain_id=pl.domain.data_ptr(),
                    B=B, NI=NI, D=D, hid=self.hid, fix_value=float(fix_value), u=pl.ev_u.data_ptr() if want_scores else None,
                    p=pl.ev_p.data_ptr() if want_scores else None, rank=pl.ev_rank.data_ptr(), rank_raw=pl.ev_rank_raw.data_ptr(),
                    loss_part=pl.ev_loss_part.data_ptr() if with_loss else None, stream=s)
        if self.dr or self.itc_bs:       # the user vectors by this model's own launches (pl.u [2, B, D]), read by the head
            # isItC at the batch sizes amid_itc_mix_fwd_f32 runs its 512-thread form on: the mix is the head's prologue, from pl.u_raw
            fold = bool(self.itc_bs and 32 <= B <= 256 and D in (64, 128))
            self._enqueue_user_vectors(pl, mix=not fold)
            mix = dict(itc_s=None, w_nn=None, b_nn=None, w_bs=None, b_bs=None, threshold=0.0, gate=None)
            if fold:
                mix = dict(itc_s=pl.itc_s.data_ptr(), w_nn=self._pp("itc_d{d}.trans_nn.weight"), b_nn=self._pp("itc_d{d}.trans_nn.bias"),
                           w_bs=self._pp("itc_d{d}.trans_bs.weight"), b_bs=self._pp("itc_d{d}.trans_bs.bias"), threshold=self.itc_threshold,
                           gate=pl.itc_gate.data_ptr())
            L.call_named("amid_eval_head_u_f32", self._scorer(), head, mix, u_src=(pl.u_raw if fold else pl.u).data_ptr(), u_dom_stride=B * D)
            return
        L.call_named("amid_eval_head_f32", self._eval_last_ln(), self._scorer(), head, x=pl.x[2].data_ptr(), T=T)

    def _eval_through_forward(self) -> bool:
        """Whether the evaluation batch's encoders are enqueue_forward's own launches (isInC: the token group in front of them)."""
        return bool(self.inc_bs)

    def _eval_last_ln(self):
        """ln_w, ln_b, eps of the LayerNorm amid_eval_head_f32 applies in front of the mean over time (null pointers: none)."""
        return dict(self._last_ln(), eps=SASREC_LN_EPS)

    def _enqueue_eval_images(self, pl: SasrecPlan) -> None:
        """The weight images the evaluation's forward reads, built once per evaluation (eval_epoch: the batches' launches only read them)."""
        if self._fwd_on_pieces(pl, pl.shape.B, pl.shape.Tenc):
            src, w16 = self._w16_images(3)
            lib().call("amid_sas_weights_bf16_planes", src, 24, self.D, 0, 3, w16.data_ptr(), self.s)

    def _enqueue_eval_encoders(self, pl: SasrecPlan, build_images: bool) -> None:
        """The sequences' rows and the inference forward of an evaluation batch, up to pl.x[2]: over the live list, or (a null list) over both
        domains of every row for a model whose head needs them.  The kernels are enqueue_forward(train=False)'s for the shape, or their
        inference twins (tests/test_gpu_eval.py)."""
        L, s, shp, D = lib(), self.s, pl.shape, self.D
        B, T = shp.B, shp.Tenc
        st = self.step_state.data_ptr()
        lf = None if self.itc_bs else pl.live.data_ptr()      # isItC: the pair-max reads both domains' rows of every sample
        pos = self._pos()
        if not L.value("amid_sas_seq_supported", B, T, D, self.H):       # eval_fused_ok said yes: the long shape (_eval_long)
            self._enqueue_eval_encoders_long(pl, lf, pos)
            return
        split = self._fwd_on_pieces(pl, B, T)
        pl.w16_written = pl.wT16x3_written = False
        # the forward's workgroups gather their own rows: three launches a batch (the gather prologue walks a live list: not without one)
        gat = bool(split and self.GATHER_ON_FWD and lf is not None)
        k1 = self._k1_head(pl, pos["pos0"], pos["pos1"], pl.tmq.data_ptr(), 0, SASREC_P_DROP, 0)      # (no candidate rows: the head gathers them)
        if gat:
            src, w16 = self._w16_images(3)
            if build_images:
                L.call("amid_sas_weights_bf16_planes", src, 24, D, 0, 3, w16.data_ptr(), s)
        elif split and build_images:          # the gather's extra workgroups write the weights' three-plane images (the forward's operands)
            src, w16 = self._w16_images(3)
            L.call_named("amid_embed_fwd_w16_f32", k1, self._w16_riders(transposes=False), table=self.table.data_ptr(), live=lf, idx_c=None, row_c=None)
        else:
            if split:
                src, w16 = self._w16_images(3)
            if lf is not None:
                L.call_named("amid_embed_fwd_live_f32", k1, table=self.table.data_ptr(), live=lf)
            else:
                L.call_named("amid_embed_fwd_f32", k1, table=self.table.data_ptr())
        fams = self._fams()
        enc = dict(n_layers=2, xout=pl.x[2].data_ptr(), ln_eps=SASREC_LN_EPS, B=B, T=T, D=D, H=self.H, live=lf, stream=s)
        if gat:
            L.call_named("amid_sas_seq_fwd_gather_infer_f32", fams, enc, pos, w16x3=w16.data_ptr(), table=self.table.data_ptr(),
                         idx_all=pl.idx_all.data_ptr())
        elif split:
            L.call_named("amid_sas_seq_fwd_split_infer_f32", fams, enc, x0=pl.x[0].data_ptr(), tmq=pl.tmq.data_ptr(), w16x3=w16.data_ptr())
        else:              # D 64 / compute = "bf16" / FWD_SPLIT off: the saving forward over the live sequences
            sv = self._seq_ptrs(pl)
            if self.compute == "bf16":
                src, w16 = self._w16_images(1)
                L.call("amid_sas_weights_bf16_planes", src, 24, D, 0, 1, w16.data_ptr(), s)
                L.call_named("amid_sas_seq_fwd_bf16w_f32", fams, enc, sv, tmq=pl.tmq.data_ptr(), step_state=st, train=0, p_drop=SASREC_P_DROP,
                             w16=w16.data_ptr())
            else:
                L.call_named("amid_sas_seq_fwd_f32", fams, enc, sv, tmq=pl.tmq.data_ptr(), step_state=st, train=0, p_drop=SASREC_P_DROP)

    def _enqueue_eval_encoders_long(self, pl: SasrecPlan, lf, pos) -> None:
        """64 < T <= 256: six launches up to pl.x[2], in the plan's q / k / v / o buffers; no gathered rows, nothing saved for a backward."""
        L, s, shp, D = lib(), self.s, pl.shape, self.D
        lay = self._lay()
        dims = dict(B=shp.B, T=shp.Tenc, D=D, live=lf, stream=s)
        L.call_named("amid_sas_strip_qkv_fwd_gather_infer_f32", pos, self._qkv_block(pl, 0), dims, table=self.table.data_ptr(), idx_all=pl.idx_all.data_ptr(),
                     ln_eps=SASREC_LN_EPS, tmq=pl.tmq.data_ptr())
        for l in (0, 1):
            L.call_named("amid_attn_fwd_long_live_infer_f32", dims, q=pl.q[l].data_ptr(), k=pl.k[l].data_ptr(), v=pl.v[l].data_ptr(), H=self.H,
                         o=pl.o[l].data_ptr())
            nxt = self._qkv_block(pl, 1, "n") if l == 0 else NO_NEXT_QKV
            L.call_named("amid_sas_strip_oproj_ffn_fwd_infer_f32", lay[l], nxt, dims, o=pl.o[l].data_ptr(), qn=pl.qn[l].data_ptr(),
                         ln_w=lay[l]["ln2_w"], ln_b=lay[l]["ln2_b"], tmq=pl.tmq.data_ptr(), ln_eps=SASREC_LN_EPS,
                         xo=None if l == 0 else pl.x[2].data_ptr())

    def capture_eval(self, pl: SasrecPlan, fix_value: float, with_loss: bool = True) -> None:
        """The evaluation batch as a hipGraph over the plan's static inputs (parameters are read at replay time and the forward's weight
        images are rebuilt by eval_epoch before its first replay: the graph stays valid across training steps; keyed by fix_value / with_loss)."""
        L = lib()
        self.enqueue_eval(pl, fix_value, with_loss)           # warm-up outside capture (dynamic-LDS attributes, code objects; builds the images)
        self.sync()
        L.call("amid_graph_capture_begin", self.s)
        try:
            self.enqueue_eval(pl, fix_value, with_loss, build_images=False)
        finally:
            out = ctypes.c_void_p()
            L.call("amid_graph_capture_end", self.s, ctypes.byref(out))
        if not hasattr(pl, "eval_graphs"):
            pl.eval_graphs = {}
        pl.eval_graphs[(float(fix_value), bool(with_loss))] = out.value

    def eval_epoch(self, pl: SasrecPlan, packed: torch.Tensor, fix_value: float, with_loss: bool = True, use_graph: bool = True) -> torch.Tensor:
        """Every batch of `packed` ([n_batches, in_words] int64: pack_epoch's images, resident in HBM) through the evaluation launches:
        one device copy of the image into the plan's static inputs, one graph replay, one device copy of the 3 B result words out.
        Returns [n_batches, 3 B] int32 (rank | rank_raw | loss_part bits) on the device; nothing is read back here."""
        if packed.dtype != torch.int64 or packed.dim() != 2 or packed.shape[1] != pl.in_words:
            raise ValueError(f"eval_epoch takes [n, {pl.in_words}] int64 batch images (pack_epoch)")
        if self.table_m is not None:
            self.flush_table()                   # rows with pending zero-gradient Adam steps must be current for evaluation
        out = torch.empty(packed.shape[0], 3 * pl.shape.B, dtype=torch.int32, device=self.device)
        key = (float(fix_value), bool(with_loss))
        if use_graph and key not in getattr(pl, "eval_graphs", {}):
            with torch.cuda.stream(self.stream):
                pl.in_pack.copy_(packed[0], non_blocking=True)
            self.capture_eval(pl, fix_value, with_loss)
        L = lib()
        with torch.cuda.stream(self.stream):
            self._enqueue_eval_images(pl)      # this evaluation's weight images, once (the batches' launches only read them)
            for i in range(packed.shape[0]):
                pl.in_pack.copy_(packed[i], non_blocking=True)
                if use_graph:
                    L.call("amid_graph_launch", pl.eval_graphs[key], self.s)
                else:
                    self.enqueue_eval(pl, fix_value, with_loss, build_images=False)
                out[i].copy_(self._eval_out(pl), non_blocking=True)
        return out

    # ------------------------------------------------------------------ full-catalog evaluation and top-K (csrc/full_rank.hip)
    # The user vectors come from the launches the sampled evaluation runs for this model (enqueue_eval's own-domain pl.ev_u -- for isItC
    # the mixed vector --, enqueue_forward's pl.u where eval_fused_ok says no), so the full-catalog scores are the bits test() would give the
    # same candidates.
    def enqueue_user_vectors(self, pl: SasrecPlan, fix_value: float = 0.0, build_images: bool = True):
        """The user vectors of the batch loaded into `pl` (load_batch with labels and domain ids), on the engine's stream.  Returns
        (tensor, dom_stride): user b's vector starts dom_stride * domain[b] + b * D floats into the tensor.  build_images=False: the
        fused evaluation's weight images are current (topk_epoch builds them once for all its batches, as eval_epoch does)."""
        if self.eval_fused_ok(pl):
            self.enqueue_eval(pl, fix_value, with_loss=False, want_scores=True, build_images=build_images)
            return pl.ev_u, 0
        self.enqueue_prepare(pl, sparse=False)
        self.enqueue_forward(pl, train=False, with_loss=False)
        return pl.u, pl.shape.B * self.D

    def _full_rank_workspace(self, B: int, n1: int, n2: int, k: int) -> torch.Tensor:
        nbytes = int(lib().value("amid_full_rank_workspace_bytes", B, n1, n2, self.hid, k))
        if nbytes < 0:
            raise ValueError(f"full rank / top-K: bad sizes B {B}, pools {n1} / {n2}, k {k}")
        ws = getattr(self, "_fr_ws", None)
        if ws is None or ws.numel() < nbytes:
            if ws is not None:
                ws.record_stream(self.stream)          # (launches still queued on the engine's stream may read the old one)
            with torch.cuda.stream(self.stream):
                ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._fr_ws = ws
        return ws

    def enqueue_full_rank(self, pl: SasrecPlan, pos: torch.Tensor, domain: torch.Tensor, pools, own: Optional[torch.Tensor],
                          own_off: Optional[torch.Tensor], rows: Optional[torch.Tensor], fix_value: float, rank: torch.Tensor,
                          rank_raw: torch.Tensor, scores: Optional[torch.Tensor] = None) -> None:
        """test()'s rank of the positive against the WHOLE pool of its domain minus the row's own items (the set its negatives are drawn
        from, dataset_seq.py:188 / :206), for the batch loaded into `pl`: rank / rank_raw [B] int32 (with fix_value / with 0).  pos,
        domain [B] int64; pools (pool_d1, pool_d2) sorted unique int64; own / own_off / rows: DeviceBatches.own, .own_off and the
        batch's dataset row ids (int32), or None.  scores [B, >= max pool] optional (tests).  Nothing is synchronised."""
        u, stride = self.enqueue_user_vectors(pl, fix_value)
        B = pl.shape.B
        p1, p2 = pools
        ws = self._full_rank_workspace(B, p1.numel(), p2.numel(), 0)
        lib().call_named("amid_full_rank_f32", self._scorer(), self._catalog(domain, pools, own, own_off, rows), u=u.data_ptr(), u_dom_stride=stride,
                         pos=pos.data_ptr(), B=B, fix_value=float(fix_value), workspace=ws.data_ptr(), flags=pl.err.data_ptr(), rank=rank.data_ptr(),
                         rank_raw=rank_raw.data_ptr(), scores=None if scores is None else scores.data_ptr(),
                         n_cols=0 if scores is None else scores.shape[1])

    def _catalog(self, domain: torch.Tensor, pools, own, own_off, rows):
        """What the full-catalog launches score against: the rows' domains, the two pools, the rows' own items (or None), the table."""
        ptr = lambda t: None if t is None else t.data_ptr()       # noqa: E731
        p1, p2 = pools
        return dict(domain_id=domain.data_ptr(), pool_d1=p1.data_ptr(), n_pool_d1=p1.numel(), pool_d2=p2.data_ptr(), n_pool_d2=p2.numel(),
                    own_items=ptr(own), own_off=ptr(own_off), rows=ptr(rows), table=self.table.data_ptr(), n_rows=self.n_rows, D=self.D,
                    hid=self.hid, stream=self.s)

    def enqueue_topk(self, pl: SasrecPlan, domain: torch.Tensor, pools, own: Optional[torch.Tensor], own_off: Optional[torch.Tensor],
                     rows: Optional[torch.Tensor], k: int, exclude_history: bool, ids: torch.Tensor, scores: torch.Tensor) -> None:
        """The k best candidates of every row's domain pool (minus its own items with exclude_history) for the batch loaded into `pl`:
        ids [B, k] int64 / scores [B, k], best first, ties to the lower id, padded with -1 / -inf.  Arguments as enqueue_full_rank."""
        u, stride = self.enqueue_user_vectors(pl)
        B = pl.shape.B
        p1, p2 = pools
        ws = self._full_rank_workspace(B, p1.numel(), p2.numel(), int(k))
        lib().call_named("amid_topk_f32", self._scorer(), self._catalog(domain, pools, own, own_off, rows), u=u.data_ptr(), u_dom_stride=stride, B=B,
                         top_k=int(k), exclude_history=1 if exclude_history else 0, workspace=ws.data_ptr(), flags=pl.err.data_ptr(), ids=ids.data_ptr(),
                         scores=scores.data_ptr())

    # ------------------------------------------------------------------ the encode / score split and neighbours (csrc/neighbors.hip)
    def encode_epoch(self, pl: SasrecPlan, packed: torch.Tensor, use_graph: bool = True) -> torch.Tensor:
        """The vector topk_epoch scores for every row of `packed` ([n, in_words] int64: pack_epoch's images, resident in HBM), as
        [n, 1, B, D] float32 on the device (enqueue_user_vectors' own-domain vectors; isItC: the mixed ones) or [n, 2, B, D] (the
        forward's vectors of both domains where the evaluation is not fused: row b's is [domain(b) != 0]).  The lazy table flushed and the
        weight images built once, then per batch one device copy of the image, one graph replay of enqueue_user_vectors (use_graph=False:
        the same launches, eagerly) and one device copy out.  Nothing is read back."""
        if packed.dtype != torch.int64 or packed.dim() != 2 or packed.shape[1] != pl.in_words:
            raise ValueError(f"encode_epoch takes [n, {pl.in_words}] int64 batch images (pack_epoch)")
        if self.table_m is not None:
            self.flush_table()
        L = lib()
        n, B, D = packed.shape[0], pl.shape.B, self.D
        fused = self.eval_fused_ok(pl)
        with torch.cuda.stream(self.stream):
            if fused:
                self._enqueue_eval_images(pl)
        if use_graph and getattr(pl, "enc_graph", None) is None:
            with torch.cuda.stream(self.stream):
                pl.in_pack.copy_(packed[0], non_blocking=True)
                self.enqueue_user_vectors(pl)                # warm-up outside capture (LDS attributes, lazy buffers, images)
            self.sync()
            L.call("amid_graph_capture_begin", self.s)
            try:
                self.enqueue_user_vectors(pl, build_images=False)
            finally:
                out = ctypes.c_void_p()
                L.call("amid_graph_capture_end", self.s, ctypes.byref(out))
            pl.enc_graph = out.value
        two = not fused                                      # enqueue_user_vectors' rule: the forward's [2, B, D] where the evaluation is not fused
        raw = torch.empty(n, 2 if two else 1, B, D, dtype=torch.float32, device=self.device)
        self.stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self.stream):
            for i in range(n):
                pl.in_pack.copy_(packed[i], non_blocking=True)
                if use_graph:
                    L.call("amid_graph_launch", pl.enc_graph, self.s)
                    u = pl.u if two else pl.ev_u
                else:
                    u, stride = self.enqueue_user_vectors(pl, build_images=False)
                    assert (stride != 0) == two
                raw[i].view(-1).copy_(u.reshape(-1)[:raw[i].numel()], non_blocking=True)
        return raw

    def enqueue_topk_vectors(self, u: torch.Tensor, domain: torch.Tensor, pools, history: Optional[torch.Tensor], k: int,
                             ids: torch.Tensor, scores: torch.Tensor, err: torch.Tensor) -> None:
        """amid_topk_f32 on caller-supplied vectors u [B, D] (u_dom_stride = 0; any B): the k best candidates of every row's domain pool,
        minus the ids of history [B, T] (int64; amid_own_from_seq_i64 forms the sets on the device) when given.  err: [1] int32 flags.
        Nothing is synchronised."""
        L, B = lib(), u.shape[0]
        p1, p2 = pools
        ws = self._full_rank_workspace(B, p1.numel(), p2.numel(), int(k))
        own = own_off = rows = None
        if history is not None:
            T = history.shape[1]
            with torch.cuda.stream(self.stream):
                own = torch.empty(B * T, dtype=torch.int64, device=self.device)
                own_off = torch.empty(B + 1, dtype=torch.int32, device=self.device)
                cnt = torch.empty(B, dtype=torch.int32, device=self.device)
                rows = torch.arange(B, dtype=torch.int32, device=self.device)
            L.call("amid_own_from_seq_i64", history.data_ptr(), history.data_ptr(), domain.data_ptr(), B, T, cnt.data_ptr(), own.data_ptr(),
                   own_off.data_ptr(), self.s)
        L.call_named("amid_topk_f32", self._scorer(), self._catalog(domain, pools, own, own_off, rows), u=u.data_ptr(), u_dom_stride=0, B=B, top_k=int(k),
                     exclude_history=0 if history is None else 1, workspace=ws.data_ptr(), flags=err.data_ptr(), ids=ids.data_ptr(),
                     scores=scores.data_ptr())

    NEIGHBOR_METRICS = {"dot": 0, "cosine": 1}

    def flags_holder(self):
        """A [1] int32 flag word for launches that belong to no plan (check_index_error takes it like a plan)."""
        if getattr(self, "_flag_holder", None) is None:
            with torch.cuda.stream(self.stream):
                self._flag_holder = types.SimpleNamespace(err=torch.zeros(1, dtype=torch.int32, device=self.device))
        return self._flag_holder

    def enqueue_neighbors(self, queries: torch.Tensor, base: torch.Tensor, pool: Optional[torch.Tensor], metric: str, k: int,
                          exclude_self: bool, ids: torch.Tensor, scores: torch.Tensor, err: torch.Tensor) -> None:
        """amid_neighbors_f32 on the engine's stream: queries [Q] int64 (rows of base) or [Q, D] float32 vectors against the rows `pool`
        (sorted unique int64, None: every row) of base [N, D] (contiguous float32, D 64 / 128); ids [Q, k] int64, scores [Q, k].
        Nothing is synchronised."""
        by_id = queries.dtype == torch.int64
        Q, (N, D) = queries.shape[0], base.shape
        n_cand = N if pool is None else pool.numel()
        nbytes = int(lib().value("amid_neighbors_workspace_bytes", Q, n_cand, D, int(k)))
        if nbytes < 0:
            raise ValueError(f"neighbors: bad sizes Q {Q}, candidates {n_cand}, D {D}, k {k}")
        ws = getattr(self, "_nb_ws", None)
        if ws is None or ws.numel() < nbytes:
            if ws is not None:
                ws.record_stream(self.stream)
            with torch.cuda.stream(self.stream):
                ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._nb_ws = ws
        lib().call("amid_neighbors_f32", None if by_id else queries.data_ptr(), queries.data_ptr() if by_id else None, Q, base.data_ptr(), N, D,
                   None if pool is None else pool.data_ptr(), n_cand, self.NEIGHBOR_METRICS[metric], int(k), 1 if exclude_self else 0,
                   ws.data_ptr(), err.data_ptr(), ids.data_ptr(), scores.data_ptr(), self.s)

    # ------------------------------------------------------------------ parameter interchange
    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        with torch.no_grad(), torch.cuda.stream(self.stream):
            self.table.copy_(sd["item_emb_layer.emb_item.weight"].to(self.device, torch.float32))
            for name in self.dense.slots:
                self.dense.view(name).copy_(sd[name].to(self.device, torch.float32))
        self.sync()

    def state_dict(self) -> Dict[str, torch.Tensor]:
        out = {"item_emb_layer.emb_item.weight": self.table}
        for name in self.dense.slots:
            out[name] = self.dense.view(name)
        return out

    def check_index_error(self, pl: SasrecPlan) -> None:
        flags = int(pl.err.item())
        if flags != 0:
            pl.err.zero_()
            if flags & 2:      # AMID_FLAG_UMAX_EXCEEDED
                raise RuntimeError("amid_amd: a data-parallel step found more unique rows than the bound umax it was given "
                                   "(train_step_dp): its exchange chunk is corrupt")
            raise IndexError("amid_amd: item index out of range in the batch (nn.Embedding would raise here, model_seq.py:27-29)")
