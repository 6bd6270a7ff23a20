"""Time GRU4Rec's train step and evaluation batch (amid_amd.model_gru.GRU4Rec / GRU4RecAMID: csrc/gru.hip under engine_gru.py).

    python profiles/tools/gru4rec_time.py [--batches 16] [--windows 5] [--min_s 0.5] [--only T50_train] [--variants plain,itc,inc,inc_itc,itc_dr]

GRU4Rec, D 128, hid 32, the reference-sized table of 894 820 rows, random weights; B 256 rows a batch, left-padded sequences of 1 .. T ids
drawn uniformly from the table, one negative a row for training and 99 for evaluation.  Four configurations, alternating window by window:
  * T50_train / T20_train: pool_step() on an epoch pool of --batches batches -- one graph replay a step, the live sequences only
  * T50_eval / T20_eval:   the engine's eval_epoch() (what eval_ranks() runs) over --batches packed batches -- one graph replay a batch
A window repeats its configuration's whole set of batches until --min_s has passed and ends in a device synchronise (host clock,
time.perf_counter); printed: ms per step / batch of every window, median, spread (max - min).
--variants: the models to time side by side in ONE run, every configuration of every variant alternating window by window (plain: GRU4Rec;
itc / inc / inc_itc / itc_dr: GRU4RecAMID with isItC / isInC / both / isItC + isDR at bs = B, thresholds 1 / B so that the gates are
mixed; itc_dr trains objective 0 on Adam state 0).  Their configurations are named VARIANT_T50_train, ...; plain alone keeps the short names.
Kernel-level splits: run it under `rocprofv3 --kernel-trace --stats -- python profiles/tools/gru4rec_time.py --windows 1 --min_s 0.05 --only T50_train`.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from amid_amd.model_gru import GRU4Rec, GRU4RecAMID  # noqa: E402

N_ROWS, D, HID, B = 894820, 128, 32, 256
VARIANTS = {"plain": (False, False, False), "itc": (False, True, False), "inc": (True, False, False), "inc_itc": (True, True, False),
            "itc_dr": (False, True, True)}           # (isInC, isItC, isDR)


def make(variant, T, **kw):
    inc, itc, dr = VARIANTS[variant]
    if variant == "plain":
        return GRU4Rec(10, D, N_ROWS, D, T, HID, B, False, False, 0.5, 0.5, **kw)
    return GRU4RecAMID(10, D, N_ROWS, D, T, HID, B, inc, itc, 1.0 / B, 1.0 / B, isDR=dr, **kw)


def epoch(n, T, neg, seed, dev):
    g = torch.Generator().manual_seed(seed)
    pad = N_ROWS - 1

    def seq():
        ids = torch.randint(1, pad, (n, B, T), generator=g)
        n_pad = torch.randint(0, T, (n, B, 1), generator=g)
        return torch.where(torch.arange(T) < n_pad, torch.full_like(ids, pad), ids)

    label = torch.zeros(B, 1 + neg)
    label[:, 0] = 1.0
    ep = dict(i_node=torch.randint(1, pad, (n, B), generator=g), neg_samples=torch.randint(1, pad, (n, B, neg), generator=g), seq_d1=seq(),
              seq_d2=seq(), domain_id=torch.randint(0, 2, (n, B), generator=g), ob_label=torch.randint(0, 2, (n, B), generator=g), label=label)
    return {k: v.to(dev) for k, v in ep.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--min_s", type=float, default=0.5)
    ap.add_argument("--only", type=str, default="", help="one configuration (T50_train, T20_train, T50_eval, T20_eval)")
    ap.add_argument("--variants", type=str, default="plain", help="comma-separated: " + ", ".join(VARIANTS))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    n = args.batches
    configs = {}
    variants = args.variants.split(",")
    for variant in variants:
        pre = "" if variants == ["plain"] else variant + "_"
        for T in (50, 20):
            if args.only and not args.only.startswith(f"{pre}T{T}_"):
                continue
            model = make(variant, T, lr=5e-4, seed=1)
            tr, ev = epoch(n, T, 1, 10 + T, dev), epoch(n, T, 99, 20 + T, dev)

            model.begin_epoch_pool(tr)                   # installed once: pool_step() walks it round and round by the device step counter
            # (a model of its own that never trains: eval_epoch() then has no lazily-updated table rows to flush first)
            eng = make(variant, T, seed=2).engine
            pl = eng.plan(B, T, 100, need_grad=False)
            packed = eng.pack_epoch(pl, ev["i_node"], ev["neg_samples"], ev["seq_d1"], ev["seq_d2"], ev["label"], ev["domain_id"])
            torch.cuda.synchronize()

            def train(model=model):
                for _ in range(n):
                    model.pool_step()

            def evaluate(eng=eng, pl=pl, packed=packed):
                eng.eval_epoch(pl, packed, 1e-7, with_loss=True, use_graph=True)

            configs[f"{pre}T{T}_train"], configs[f"{pre}T{T}_eval"] = train, evaluate
    if args.only:
        configs = {args.only: configs[args.only]}
    for fn in configs.values():                      # warm-up of every configuration (captures its graph)
        fn()
    torch.cuda.synchronize()
    ms = {c: [] for c in configs}
    for _ in range(args.windows):
        for c, fn in configs.items():
            torch.cuda.synchronize()
            t0, reps = time.perf_counter(), 0
            while True:
                fn()
                reps += 1
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if dt >= args.min_s:
                    break
            ms[c].append(dt * 1e3 / (reps * n))
    for c, w in ms.items():
        print(json.dumps({"config": c, "B": B, "D": D, "batches": n, "clock": "host perf_counter around synchronised windows",
                          "ms": [round(x, 5) for x in w], "median": round(statistics.median(w), 5), "spread": round(max(w) - min(w), 5)}),
              flush=True)


if __name__ == "__main__":
    main()
