"""Training driver with the reference's ``train_sr.py`` command line (train_sr.py:357-625), running the hot
loop on the MI355X engine.

Same flags as the reference (train_sr.py:360-389; the ones the reference never reads are accepted and
ignored; ``type=bool`` flags keep the reference's "any non-empty string is True" behaviour), same
constants (item_length 447 410, pad id item_length + 1, table of 2 x item_length rows, drop_last on both
loaders, five seeds 0..4, loss logged every 20 iterations, best-so-far HR/NDCG/MRR per epoch).
Additions: ``--data_root`` (the reference hard-codes /ossfs/workspace/CDSR), ``--seeds``, ``--device``,
``--no_graph``, ``--no_pool``, ``--max_steps``, ``--dtype {fp32,bf16}``, ``--neg_sampling {uniform,popularity}`` with ``--neg_power P``
(0 .. 1, default 1.0) and ``--neg_sampling_for {both,train,eval}`` (negatives drawn in proportion to count ** P in the training CSV
instead of uniformly: DESIGN.md section 16), ``--train_negs K`` (1 .. 1023 sampled negatives a training row, default 1) with
``--loss {bce,softmax,bpr}`` (the objective over the row's positive and its K negatives; default the reference's masked BCE; softmax / bpr:
one GPU, fp32, no --isInC: DESIGN.md section 17), ``--hard_negs H`` with ``--hard_skip S`` (train on the H of the K drawn negatives that the current
model ranks S .. S + H - 1 by logit: DESIGN.md section 18); data parallel when launched by ``python -m torch.distributed.run --nproc-per-node N``
(one process per GPU, RCCL, ``--bs`` per GPU; BASELINE.json configs[3]).

    python train_sr.py --data_root /path/to/AMID -ds amazon -dm cloth_sport --overlap_ratio 0.75 \
        --model sasrec --bs 256 --seq_len 50 --emb_dim 128 --epoch 2 --seeds 1
"""
from __future__ import annotations

import argparse
import logging
import os
import random
import time

import numpy as np
import torch

from .dataset_seq import DeviceBatches, DualDomainSeqDataset, JointBatches, item_counts
from .model_gru import GRU4Rec, GRU4RecAMID
from .model_seq import BERT4Rec, SASRec
from .utils import AverageMeter, device_positive_ranks, init_logger, scores_from_ranks

logger = logging.getLogger()
FIX_VALUE = 1e-7          # train_sr.py:42: ties between the positive and a negative count against the positive


STEPS_PER_GRAPH = 4          # train(): consecutive pooled steps per replayed hipGraph (single GPU)


class _NegFlag(argparse.Action):
    """Stores the value and notes that the flag was given (check_neg_sampling: --neg_power / --neg_sampling_for need popularity)."""

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, values)
        namespace.neg_flags_given = namespace.neg_flags_given + (option_string,)


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Multi-edge multi-domain training")
    p.add_argument("--epoch", type=int, default=50, help="# of epoch")
    p.add_argument("--bs", type=int, default=256, help="# images in batch")
    p.add_argument("--use_gpu", type=bool, default=True)
    p.add_argument("--lr", type=float, default=5e-4, help="initial learning rate for adam")
    p.add_argument("--emb_dim", type=int, default=128, help="embedding size")
    p.add_argument("--hid_dim", type=int, default=32, help="hidden layer dim")
    p.add_argument("--seq_len", type=int, default=20, help="the length of the sequence")
    p.add_argument("--graph_nums", type=int, default=2)
    p.add_argument("--head_nums", type=int, default=32)
    p.add_argument("--long_length", type=int, default=7, help="the length for setting long-tail node")
    p.add_argument("--m1_layers", type=int, default=3)
    p.add_argument("--m2_layers", type=int, default=3)
    p.add_argument("--m3_layers", type=int, default=4)
    p.add_argument("--m4_layers", type=int, default=2)
    p.add_argument("--alpha_l", type=int, default=3)
    p.add_argument("--neg_nums", type=int, default=199, help="sample negative numbers")
    p.add_argument("--mask_rate_enc", type=float, default=0.9)
    p.add_argument("--mask_rate_dec", type=float, default=0.9)
    p.add_argument("--overlap_ratio", type=float, default=0.5, help="overlap ratio for choose dataset")
    p.add_argument("--bs_ratio", type=float, default=0.5)
    p.add_argument("-md", "--model-dir", type=str, default="model/")
    p.add_argument("--log-file", type=str, default="log")
    p.add_argument("--model", type=str, default="model select")
    p.add_argument("-ds", "--dataset_type", type=str, default="amazon")
    p.add_argument("-dm", "--domain_type", type=str, default="movie_book")
    p.add_argument("--isInC", type=bool, default=False, help="add inc")
    p.add_argument("--isItC", type=bool, default=False, help="add itc")
    p.add_argument("--ts1", type=float, default=0.5)
    p.add_argument("--ts2", type=float, default=0.5)
    p.add_argument("--overlap", type=bool, default=False, help="split the metrics by overlapped / non-overlapped users")
    # additions
    p.add_argument("--data_root", type=str, default=".", help="directory holding {amazon,mybank}_dataset/ (reference: /ossfs/workspace/CDSR)")
    p.add_argument("--seeds", type=int, default=5, help="number of seeds 0..n-1 (reference: 5)")
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--no_graph", action="store_true", help="launch the step eagerly instead of replaying a hipGraph")
    p.add_argument("--no_pool", action="store_true", help="build and copy every batch inside the loop (the reference's way) instead of "
                                                          "keeping the epoch's packed batches resident in HBM")
    p.add_argument("--max_steps", type=int, default=0, help="stop each epoch after this many steps (0 = full epoch)")
    p.add_argument("--dtype", type=str, default="fp32", choices=("fp32", "bf16"),
                   help="fp32: exact fp32 matrix products; bf16: bf16 MFMA operands, fp32 accumulation and storage (sasrec, emb_dim 128)")
    p.add_argument("--full_rank", action="store_true", help="also rank every positive against its domain's whole item pool (minus the "
                                                            "user's own items) and log those metrics as d1_full / d2_full")
    p.add_argument("--neg_sampling", type=str, default="uniform", choices=("uniform", "popularity"),
                   help="uniform: negatives uniform over pool minus own (the reference); popularity: in proportion to count ** --neg_power, "
                        "counted in the training CSV, without replacement")
    p.add_argument("--neg_power", type=float, default=1.0, action=_NegFlag, help="--neg_sampling popularity: 0 .. 1 (0 is uniform)")
    p.add_argument("--neg_sampling_for", type=str, default="both", choices=("both", "train", "eval"), action=_NegFlag,
                   help="--neg_sampling popularity: which loaders draw that way (the others stay uniform)")
    p.set_defaults(neg_flags_given=())
    p.add_argument("--train_negs", type=int, default=1, metavar="K", help="sampled negatives per training row, 1 .. 1023 (the reference: 1)")
    p.add_argument("--loss", type=str, default="bce", choices=("bce", "softmax", "bpr"),
                   help="the training objective over a row's positive and its --train_negs negatives: the reference's masked BCE, sampled "
                        "softmax, or BPR (the validation loss stays the BCE)")
    p.add_argument("--hard_negs", type=int, default=0, metavar="H",
                   help="with --loss softmax | bpr: train on the H hardest (highest-scoring under the current model) of the --train_negs drawn "
                        "negatives a row (0: on all of them)")
    p.add_argument("--hard_skip", type=int, default=0, metavar="S",
                   help="with --hard_negs: leave out the S highest-scoring negatives (often false negatives) and keep the H after them")
    p.add_argument("--save_dir", type=str, default=None,
                   help="write DIR/seed{i}/best_d1.pt and best_d2.pt (weights only, kept when MRR_d1 / MRR_d2 >= the best so far; held as "
                        "device copies until the seed's run ends: two extra table-sized buffers in HBM) and DIR/seed{i}/last.pt (the "
                        "whole training state, for --resume)")
    p.add_argument("--save_every", type=int, default=0, help="with --save_dir: write last.pt every N epochs (0: after the seed's last epoch only)")
    p.add_argument("--resume", type=str, default=None, help="continue the seed of this last.pt at its next epoch, then run the remaining seeds")
    return p


# what a last.pt must share with the command line that resumes it
RESUME_KEYS = ("model", "emb_dim", "seq_len", "hid_dim", "isItC", "isInC", "dtype", "dataset_type", "domain_type", "bs", "overlap_ratio",
               "neg_sampling", "neg_power", "neg_sampling_for", "train_negs", "loss", "hard_negs", "hard_skip")
_FLAGS = {"dataset_type": "-ds", "domain_type": "-dm"}
# what a last.pt written before a key existed counts as
_RESUME_DEFAULTS = {"neg_sampling": "uniform", "neg_power": 1.0, "neg_sampling_for": "both", "train_negs": 1, "loss": "bce",
                    "hard_negs": 0, "hard_skip": 0}


def check_neg_sampling(args) -> None:
    """--neg_sampling / --neg_power / --neg_sampling_for against each other: SystemExit before any GPU work."""
    if args.neg_sampling != "popularity" and args.neg_flags_given:
        raise SystemExit(f"{args.neg_flags_given[0]} belongs to --neg_sampling popularity")
    if not 0.0 <= args.neg_power <= 1.0:
        raise SystemExit(f"--neg_power must be in 0..1, got {args.neg_power}")


def check_train_loss(args) -> None:
    """--train_negs / --loss / --hard_negs / --hard_skip against the other flags: SystemExit before any GPU work."""
    if not 1 <= args.train_negs <= 1023:
        raise SystemExit(f"--train_negs must be in 1..1023, got {args.train_negs}")
    if args.loss != "bce" and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit(f"--loss {args.loss} trains on one GPU: the data-parallel listwise step is not built")
    if args.loss != "bce" and args.dtype == "bf16":
        raise SystemExit(f"--loss {args.loss} runs in fp32: --dtype bf16 is not built for it")
    if args.hard_negs < 0 or args.hard_skip < 0:
        raise SystemExit(f"--hard_negs and --hard_skip must be >= 0, got {args.hard_negs} and {args.hard_skip}")
    if args.hard_negs > 0 and args.loss == "bce":
        raise SystemExit("--hard_negs needs --loss softmax or bpr: the masked BCE has nothing to mine")
    if args.hard_skip > 0 and args.hard_negs == 0:
        raise SystemExit("--hard_skip belongs to --hard_negs")
    if args.hard_skip + args.hard_negs > args.train_negs:
        raise SystemExit(f"--hard_skip + --hard_negs = {args.hard_skip + args.hard_negs} exceeds the --train_negs {args.train_negs} drawn a row")


def neg_loader_args(args, role: str, ds=None, ds_train=None) -> dict:
    """DeviceBatches' negatives / counts / power for a loader of `role` ("train" | "eval").  A training loader weighs by its own
    dataset's counts; an evaluation loader over `ds` by the training dataset's (`ds_train`), mapped onto its pools by id."""
    if args.neg_sampling != "popularity" or args.neg_sampling_for not in ("both", role):
        return {}
    counts = item_counts(ds_train, onto=ds.pool) if role == "eval" else None
    return {"negatives": "popularity", "counts": counts, "power": args.neg_power}


def run_signature(args, keys=RESUME_KEYS) -> dict:
    return {k: getattr(args, k) for k in keys}


def read_resume(args, keys=RESUME_KEYS):
    """--save_dir / --resume, before any GPU work: refused under data parallel; the --resume file (read to the CPU) must come from a
    run of this command line -- SystemExit naming the first flag that differs.  Returns the file's contents, or None."""
    if (args.save_dir or args.resume) and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("--save_dir / --resume are single-GPU only: data-parallel replicas differ in their dropout seeds")
    if not args.resume:
        return None
    ck = torch.load(args.resume, map_location="cpu", weights_only=True)
    saved = ck.get("extra", {}).get("args", {})
    for k, v in run_signature(args, keys).items():
        was = saved.get(k, _RESUME_DEFAULTS.get(k))
        if was != v:
            raise SystemExit(f"--resume {args.resume}: {_FLAGS.get(k, '--' + k)} is {v!r} here but {was!r} in the file")
    return ck


def _save_atomic(obj, path: str) -> None:
    torch.save(obj, path + ".tmp")
    os.replace(path + ".tmp", path)          # an interrupted write leaves the previous file whole


class BestModels:
    """The reference's best_d1.pt / best_d2.pt (train_sr.py:181-186, :326-332: the model is saved when MRR_d{1,2} >= the best so far)
    as device-to-device copies of the table and the flat dense buffer -- two spare table-sized buffers in HBM -- written to disk once,
    when the seed's run ends: an epoch of cloth_sport_train25 with its evaluation takes 0.04 s, a 894 820 x 128 table is 458 MB."""

    def __init__(self, model):
        self.model, self.copies, self.mrr, self.epoch = model, {}, {}, {}

    def snapshot(self, d: str) -> None:
        """The model's current weights into domain d's spare buffers (allocated on first use)."""
        eng = self.model.engine
        if d not in self.copies:
            self.copies[d] = (torch.empty_like(eng.table), torch.empty_like(eng.dense.data))
        eng.flush_table()                 # (the evaluation that judged these weights has flushed already)
        with torch.cuda.stream(eng.stream):
            self.copies[d][0].copy_(eng.table)
            self.copies[d][1].copy_(eng.dense.data)

    def offer(self, res, epoch: int) -> None:
        for d in ("d1", "d2"):
            mrr = res[d][6]
            if mrr >= self.mrr.get(d, 0.0):
                self.snapshot(d)
                self.mrr[d], self.epoch[d] = mrr, epoch

    def weights(self, d: str) -> dict:
        """{state_dict key: CPU fp32 tensor} of domain d's copy (what SASRec.state_dict() gave when it was taken)."""
        eng = self.model.engine
        eng.sync()
        table, data = self.copies[d]
        with torch.cuda.stream(eng.stream):
            out = {"item_emb_layer.emb_item.weight": table.to("cpu")}
            data = data.to("cpu")
        out.update({n: eng.dense.view(n, data).clone() for n in eng.dense.slots})
        return out

    def state(self) -> dict:
        return {d: {"mrr": self.mrr[d], "epoch": self.epoch[d], "weights": self.weights(d)} for d in sorted(self.copies)}

    def load_state(self, st: dict) -> None:
        eng = self.model.engine
        for d, s in st.items():
            self.copies[d] = (torch.empty_like(eng.table), torch.zeros_like(eng.dense.data))
            torch.cuda.synchronize(eng.device)
            w = s["weights"]
            with torch.cuda.stream(eng.stream):
                self.copies[d][0].copy_(w["item_emb_layer.emb_item.weight"])
                for n in eng.dense.slots:
                    eng.dense.view(n, self.copies[d][1]).copy_(w[n])
            self.mrr[d], self.epoch[d] = s["mrr"], s["epoch"]

    def write(self, out_dir: str) -> None:
        for d in sorted(self.copies):
            _save_atomic(self.weights(d), os.path.join(out_dir, f"best_{d}.pt"))


class RunFiles:
    """--save_dir / --save_every / --resume for one seed's run: the best models in HBM (BestModels), last.pt at epoch ends."""

    def __init__(self, args, seed: int, model, loaders: dict, summary: list, keys=RESUME_KEYS):
        self.args, self.seed, self.model, self.loaders, self.summary, self.keys = args, seed, model, loaders, summary, keys
        self.dir = os.path.join(args.save_dir, f"seed{seed}") if args.save_dir else None
        self.best_models = BestModels(model) if self.dir else None

    def resume(self, ck):
        """Load a last.pt (read_resume's) into the model, the loaders and the best-model copies; returns (next epoch, best)."""
        extra = self.model.load_training_state(ck)
        for name, ld in self.loaders.items():
            ld.load_state_dict(extra["loaders"][name])
        if self.best_models is not None:
            self.best_models.load_state(extra["best_models"])
        return int(extra["epoch"]) + 1, dict(extra["best"])

    def after_eval(self, res, epoch: int) -> None:
        if self.best_models is not None:
            self.best_models.offer(res, epoch)

    def end_epoch(self, epoch: int, best: dict, res) -> None:
        every = self.args.save_every
        if self.dir is None or not (epoch + 1 == self.args.epoch or (every > 0 and (epoch + 1) % every == 0)):
            return
        os.makedirs(self.dir, exist_ok=True)
        path = os.path.join(self.dir, "last.pt")
        self.model.save_training_state(path + ".tmp", seed=self.seed, epoch=epoch, best=dict(best), summary=list(self.summary), metrics=res,
                                       loaders={n: ld.state_dict() for n, ld in self.loaders.items()},
                                       best_models=self.best_models.state(), args=run_signature(self.args, self.keys))
        os.replace(path + ".tmp", path)

    def finish(self) -> None:
        if self.dir is not None:
            os.makedirs(self.dir, exist_ok=True)
            self.best_models.write(self.dir)


@torch.no_grad()
def test(model, args, val_batches):
    """train_sr.py:31-128: forward with neg_nums negatives, masked BCE, HR/NDCG/MRR of the positive's rank.  The rank of the
    positive is computed on the device per batch (amid_positive_rank_f32); only B ints per batch ever reach the host."""
    model.eval()
    stats = AverageMeter("loss", "loss_cls")
    ranks, ranks_raw, doms, ovs, losses = [], [], [], [], []
    # the SASRec and BERT4Rec models (plain, isDR, isItC, isInC and their combinations on one GPU): the whole evaluation set resident in HBM, per batch
    # one graph replay -- for the plain and isDR models the own domain's sequence only (the other domain's logits are never read:
    # utils.py:21-40, train_sr.py:63-64), both domains where a comp module couples them --, candidates gathered inside the scorer, BCE and
    # both ranks in the same launch (SASRec.eval_ranks / BERT4Rec's, inherited); shapes the engine does not cover go through model.forward below
    fused, ep, loader = None, None, val_batches
    if hasattr(model, "eval_ranks") and hasattr(val_batches, "epoch_tensors") and len(val_batches) > 0:
        ep = val_batches.epoch_tensors()
        fused = model.eval_ranks(ep, FIX_VALUE)
        if fused is not None:
            losses = list(fused["loss"])
            ranks, ranks_raw = [fused["rank"].reshape(-1)], [fused["rank_raw"].reshape(-1)]
            doms, ovs = [ep["domain_id"].reshape(-1)], [ep["overlap_label"].reshape(-1)]
        else:                                  # (the draw of this epoch's negatives is made: iterate the same batches)
            val_batches = [{k: (v if k == "label" else v[i]) for k, v in ep.items()} for i in range(ep["seq_d1"].shape[0])]
    for b in ([] if fused is not None else val_batches):
        outs = model(b["user_node"], b["i_node"], b["neg_samples"], b["seq_d1"], b["seq_d2"], b["long_tail_mask_d1"],
                     b["long_tail_mask_d2"], False)
        p1, p2 = outs[0], outs[1]                                                         # isDR models return six outputs
        p1, p2 = p1.reshape(len(b["i_node"]), -1), p2.reshape(len(b["i_node"]), -1)
        y = b["label"]
        m2 = b["domain_id"].float().unsqueeze(1)
        bce = torch.nn.functional.binary_cross_entropy
        losses.append((bce(p1, y, reduction="none") * (1 - m2) + bce(p2, y, reduction="none") * m2).mean())   # train_sr.py:63-64
        ranks.append(device_positive_ranks(p1, p2, b["domain_id"], FIX_VALUE))            # train_sr.py:114-115
        if args.overlap:
            ranks_raw.append(device_positive_ranks(p1, p2, b["domain_id"], 0.0))          # the overlap splits skip fix_value
            ovs.append(b["overlap_label"])
        doms.append(b["domain_id"])
    for v in torch.stack(losses).tolist():                                                # one host transfer for the epoch
        stats.update(loss=v, loss_cls=v)
    rank, dom = torch.cat(ranks), torch.cat(doms)
    out = {"loss": stats.loss, "d1": scores_from_ranks(rank[dom == 0]), "d2": scores_from_ranks(rank[dom == 1])}
    if args.overlap:
        raw, ov = torch.cat(ranks_raw), torch.cat(ovs)
        out.update(d1_ov=scores_from_ranks(raw[(dom == 0) & (ov == 1)]), d1_no=scores_from_ranks(raw[(dom == 0) & (ov == 0)]),
                   d2_ov=scores_from_ranks(raw[(dom == 1) & (ov == 1)]), d2_no=scores_from_ranks(raw[(dom == 1) & (ov == 0)]))
    if getattr(args, "full_rank", False) and ep is not None:
        # the same rows and user vectors against the domain's whole pool minus the row's own items (SASRec.full_ranks)
        fr = model.full_ranks(ep, loader, FIX_VALUE)
        rank, dom = fr["rank"].reshape(-1), ep["domain_id"].reshape(-1)
        out.update(d1_full=scores_from_ranks(rank[dom == 0]), d2_full=scores_from_ranks(rank[dom == 1]))
        if args.overlap:
            raw, ov = fr["rank_raw"].reshape(-1), ep["overlap_label"].reshape(-1)
            out.update(d1_full_ov=scores_from_ranks(raw[(dom == 0) & (ov == 1)]), d1_full_no=scores_from_ranks(raw[(dom == 0) & (ov == 0)]),
                       d2_full_ov=scores_from_ranks(raw[(dom == 1) & (ov == 1)]), d2_full_no=scores_from_ranks(raw[(dom == 1) & (ov == 0)]))
    return out


def mined_logit_means(model):
    """With --hard_negs: the mean own-domain logit of the kept and of the other sampled negatives in the last step's plan (pl.z / pl.sel
    as the step left them; one small reduction after the epoch's steps, nothing inside a step).  None without mining."""
    pl = getattr(model, "_last_plan", None)
    if pl is None or getattr(pl, "sel", None) is None or not getattr(model.engine, "hard_negs", 0):
        return None
    z, sel = pl.z, pl.sel.long()
    kept = torch.zeros_like(z, dtype=torch.bool).scatter_(1, sel, True)
    neg = z[:, 1:]
    k = kept[:, 1:]
    n_other = int(neg.shape[1] - sel.shape[1])
    mean_kept = float(neg[k].mean())
    return mean_kept, (float(neg[~k].mean()) if n_other > 0 else float("nan"))


def train(model, train_batches, args, val_batches, exchange=None, start_epoch: int = 0, best=None, files=None):
    """train_sr.py:130-355 with the loop body (:190-217) fused into model.train_step.  start_epoch / best: where a resumed run goes on
    (RunFiles.resume); files: the RunFiles of --save_dir."""
    best = {} if best is None else best
    for epoch in range(start_epoch, args.epoch):
        stats = AverageMeter("loss", "loss_cls")
        model.train()
        t0, n_samples = time.perf_counter(), 0
        pooled = not args.no_pool and hasattr(model, "begin_epoch_pool")
        # the epoch's batches resident in HBM, one graph replay per STEPS_PER_GRAPH steps (a replayed graph costs ~8 us of idle device
        # time between launches), no per-step tensor work on the host; the loss is looked at every 20 iterations as in the reference
        chunk = STEPS_PER_GRAPH if (pooled and not args.no_graph and exchange is None and not args.max_steps) else 1
        if pooled:
            n_batches = model.begin_epoch_pool(train_batches.epoch_tensors(), exchange=exchange)
            steps = ((None, None) for _ in range(n_batches))
        else:
            steps = enumerate(train_batches)
        pending = 0
        for i, (_, b) in enumerate(steps):
            if pooled:
                pending += 1
                last = i + 1 == n_batches
                if chunk > 1 and pending < chunk and not last:
                    continue                                   # the graph of `chunk` steps is replayed when its last step comes up
                if pending == chunk and chunk > 1:
                    loss = model.pool_step(use_graph=True, exchange=exchange, n_steps=chunk)
                else:
                    for _ in range(pending):                   # the epoch's tail (or chunk == 1): single-step graphs
                        loss = model.pool_step(use_graph=not args.no_graph, exchange=exchange)
                n_done, pending = pending, 0
            else:
                loss = model.train_step(b["i_node"], b["neg_samples"], b["seq_d1"], b["seq_d2"], b["label"], b["domain_id"],
                                        use_graph=not args.no_graph, exchange=exchange)
                n_done = 1
            n_samples += n_done * args.bs * (exchange.world if exchange is not None else 1)
            # the reference looks at the loss of iterations 0, 20, 40, ... (train_sr.py:217-219): logged here when the replayed chunk
            # [i + 1 - n_done, i] holds such an iteration, with the loss of the chunk's LAST step (the steps of a graph leave one loss
            # behind) -- the only host sync of the loop
            if (i // 20) * 20 > i - n_done:
                if pooled:
                    model.engine.sync()
                stats.update(loss=loss.item(), loss_cls=loss.item())
                if hasattr(model, "check_indices"):
                    model.check_indices()                                                 # nn.Embedding would have raised (model_seq.py:27-29)
                logger.info(f"train total loss:{stats.loss}, cls loss:{stats.loss_cls} \t")
            if args.max_steps and i + 1 >= args.max_steps:
                break
        if pooled:
            model.end_epoch_pool()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        logger.info(f"epoch {epoch}: {n_samples} samples in {dt:.4f} s = {n_samples / dt:.0f} samples/s (loader included)")
        mined = mined_logit_means(model)
        if mined is not None:
            logger.info(f"epoch {epoch}: hard negatives, last step: mean logit kept {mined[0]:.4f} \tnot kept {mined[1]:.4f}")
        t1 = time.perf_counter()
        res = test(model, args, val_batches)
        if files is not None:
            files.after_eval(res, epoch)
        torch.cuda.synchronize()
        n_eval = len(val_batches) * args.bs
        logger.info(f"epoch {epoch}: evaluated {n_eval} samples x {args.neg_nums + 1} candidates in {time.perf_counter() - t1:.4f} s "
                    f"= {n_eval / (time.perf_counter() - t1):.0f} samples/s")
        names = ("HR@1", "NDCG@1", "HR@5", "NDCG@5", "HR@10", "NDCG@10", "MRR")
        msg = [f"Epoch: {epoch}/{args.epoch} \tTrain Loss: {stats.loss:.4f} \tVal loss: {res['loss']:.4f}"]
        for key, sc in res.items():
            if key == "loss":
                continue
            for n, v in zip(names, sc):
                best[(key, n)] = max(best.get((key, n), 0.0), v)
            msg.append(f"val {key} cur/max " + ", ".join(f"{n}: {v:.4f}/{best[(key, n)]:.4f}" for n, v in zip(names, sc)))
        logger.info("\n".join(msg))
        if files is not None:
            files.end_epoch(epoch, best, res)
    return best


def init_data_parallel(args):
    """One process per GPU under ``python -m torch.distributed.run --nproc-per-node N train_sr.py ...`` (not in the reference, which
    is single-GPU: ``DataParallel`` is commented out at train_sr.py:473).  ``--bs`` is the batch PER GPU.  Returns (rank, world)."""
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    if world == 1:
        return 0, 1
    import torch.distributed as dist
    backend = os.environ.get("AMID_DIST_BACKEND", "nccl")            # "gloo" only for the single-GPU two-process test
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if backend == "nccl":
        args.device = f"cuda:{local}"
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device(args.device))
    else:
        dist.init_process_group(backend, rank=rank, world_size=world)
    return rank, world


def main(argv=None):
    args = build_parser().parse_args(argv)
    check_neg_sampling(args)
    check_train_loss(args)
    ck = read_resume(args)
    rank, world = init_data_parallel(args)
    summary = list(ck["extra"]["summary"]) if ck is not None else []
    for i in range(int(ck["extra"]["seed"]) if ck is not None else 0, args.seeds):
        torch.manual_seed(i); np.random.seed(i); random.seed(i)                           # train_sr.py:439-443
        args.log_file = "log" + str(i) + ".txt"
        user_length = 895510                                                              # train_sr.py:447
        item_length = 447410                                                              # train_sr.py:450
        root = os.path.join(args.data_root, f"{args.dataset_type}_dataset")
        # "-dm a+b": two datasets trained as ONE job on the shared table (BASELINE.json configs[3]): b's item
        # ids sit item_length + 2 rows behind a's (a's ids and the pad id are all <= item_length + 1), batches alternate a0 b0 a1 b1 ...
        parts = args.domain_type.split("+")
        if len(parts) > 2:
            raise SystemExit("-dm takes one dataset or two joined with '+'")
        if args.full_rank and len(parts) == 2:
            raise SystemExit(f"--full_rank with a joint job (-dm {args.domain_type}) is not supported: rank one dataset per run")
        trains, vals = [], []
        for j, dm in enumerate(parts):
            ds_train = DualDomainSeqDataset(seq_len=args.seq_len, isTrain=True, neg_nums=args.neg_nums, long_length=args.long_length,
                                            pad_id=item_length + 1, seed=i,
                                            csv_path=os.path.join(root, f"{dm}_train{int(args.overlap_ratio * 100)}.csv"))
            ds_val = DualDomainSeqDataset(seq_len=args.seq_len, isTrain=False, neg_nums=args.neg_nums, long_length=args.long_length,
                                          pad_id=item_length + 1, seed=1000 + i, csv_path=os.path.join(root, f"{dm}_test.csv"))
            if j:
                ds_train.shift_items(item_length + 2)
                ds_val.shift_items(item_length + 2)
            trains.append(DeviceBatches(ds_train, args.bs, shuffle=True, device=args.device, seed=i, rank=rank, world=world,
                                        train_negs=args.train_negs, **neg_loader_args(args, "train")))
            # (isItC under data parallel: InterComp's Linear(bs, 1) is built for the GLOBAL batch of world x --bs rows, so the
            # evaluation, which every rank runs whole, steps through batches of that size)
            vals.append(DeviceBatches(ds_val, args.bs * (world if (args.isItC or args.isInC) else 1), shuffle=False, device=args.device, seed=i,
                                      **neg_loader_args(args, "eval", ds_val, ds_train)))
        if len(parts) == 2:
            # joint mode: the second dataset's ids sit item_length + 2 rows behind the first's in the reference-sized table of
            # 2 * item_length rows (train_sr.py:456) -- checked here, on the host, before any step runs (the fused step would only flag an
            # out-of-range id at its next log point)
            top = max(int(t.ds.max_item_id()) for t in (trains[1], vals[1]))
            if top >= 2 * item_length:
                raise SystemExit(f"-dm {args.domain_type}: item id {top - (item_length + 2)} of the second dataset lands on row {top} of a "
                                 f"{2 * item_length}-row table (ids up to {item_length - 3} fit)")
        train_batches = trains[0] if len(parts) == 1 else JointBatches(*trains)
        val_batches = vals[0] if len(parts) == 1 else JointBatches(*vals)
        item_length *= 2                                                                  # train_sr.py:456 ("for pad id")
        user_length *= 2
        cls = {"gru4rec": GRU4Rec, "sasrec": SASRec, "bert4rec": BERT4Rec}.get(args.model.lower())
        if cls is None:
            raise SystemExit(f"unknown --model {args.model!r} (gru4rec | sasrec | bert4rec)")
        if cls is GRU4Rec and world > 1:
            raise SystemExit("--model gru4rec trains on one GPU: its data-parallel step is not built")
        if cls is GRU4Rec and (args.isInC or args.isItC):
            cls = GRU4RecAMID                                                              # (the plain class refuses the flags: model_gru.py)
        torch.cuda.set_device(torch.device(args.device))
        model = cls(user_length=user_length, user_emb_dim=args.emb_dim, item_length=item_length, item_emb_dim=args.emb_dim,
                    seq_len=args.seq_len, hid_dim=args.hid_dim, bs=args.bs * (world if (args.isItC or args.isInC) else 1), isInC=args.isInC, isItC=args.isItC,
                    threshold1=args.ts1,
                    threshold2=args.ts2, lr=args.lr, seed=i, **({"compute": "bf16"} if args.dtype == "bf16" else {}),
                    **({"loss": args.loss} if args.loss != "bce" else {}),
                    **({"hard_negs": args.hard_negs, "hard_skip": args.hard_skip} if args.hard_negs else {}))
        exchange = None
        if world > 1:
            # identical replicas (weights from seed i on every rank), but each rank's own dropout stream
            model.engine.set_step(model.engine.step, seed=model.engine.rank_seed(i, rank))
            from .dist import SparseDenseExchange
            n_idx = args.bs * (2 * args.seq_len + 1 + args.train_negs)                    # per-rank index count of a train batch
            exchange = SparseDenseExchange(model.engine.merge_backend(world * n_idx),
                                           host_staging=os.environ.get("AMID_DIST_BACKEND", "nccl") != "nccl")
        files = RunFiles(args, i, model, {"train": train_batches, "val": val_batches}, summary)
        start, best = 0, None
        if ck is not None:
            start, best = files.resume(ck)
            ck = None
        init_logger(args.model_dir if rank == 0 else os.path.join(args.model_dir, f"rank{rank}"), args.log_file)
        logger.info(vars(args))
        if start:
            logger.info(f"resumed from {args.resume}: seed {i} at epoch {start}")
        best = train(model, train_batches, args, val_batches, exchange, start_epoch=start, best=best, files=files)
        files.finish()
        summary.append(best)
    keys = sorted(summary[0]) if summary else []
    init_logger(args.model_dir if rank == 0 else os.path.join(args.model_dir, f"rank{rank}"), "log_all.txt")
    for k in keys:                                                                        # train_sr.py:549-569: mean / std over the seeds
        v = np.array([s[k] for s in summary])
        logger.info(f"{k[0]} {k[1]}: mean {v.mean():.4f} std {v.std():.4f}")
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()
    return summary


if __name__ == "__main__":
    main()
