"""Time an evaluation batch beyond 64 tokens with HIP events: the fused launches (SasrecEngine.eval_epoch: one graph replay a batch)
against the path those shapes took before -- test()'s per-batch model.forward + BCE + rank kernel (amid_amd/train_sr.py).

    python profiles/tools/eval_long_time.py [--reps 50] [--T 100 150] [--B 256] [--neg 999]

Plain SASRec, D 128, hid 32, random weights, synthetic batches (left-padded, short real lengths).  Both paths run in the same process on
the same batches, alternating in two windows each; prints ms per batch of B x (1 + neg) candidates.  Kernel-level splits: run it under
`rocprofv3 --kernel-trace --stats -- python profiles/tools/eval_long_time.py --reps 5`.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from oracle import amid_oracle as orc  # noqa: E402

FIX, D, HID, N_ITEMS, NB = 1e-7, 128, 32, 20000, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--T", type=int, nargs="+", default=[100, 150])
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--neg", type=int, default=999)
    args = ap.parse_args()
    from amid_amd import model_seq
    from amid_amd.utils import device_positive_ranks
    B, NI = args.B, 1 + args.neg
    bce = torch.nn.functional.binary_cross_entropy
    for T in args.T:
        model = model_seq.SASRec(10, D, N_ITEMS, D, T, HID, B, False, False, 0.5, 0.5, seed=2)
        model.eval()
        eng = model.engine
        batches = []
        for i in range(NB):
            b = orc.synthetic_batch(B, T, N_ITEMS - 1, pad_id=N_ITEMS - 1, neg=args.neg, seed=900 + i)
            b["label"] = torch.zeros(B, NI)
            b["label"][:, 0] = 1.0
            batches.append({k: v.cuda() for k, v in b.items()})
        torch.cuda.synchronize()
        pl = eng.plan(B, T, NI, need_grad=False)
        fused_ok = eng.eval_fused_ok(pl)
        packed = None
        if fused_ok:
            packed = torch.stack([eng.pack_batch(pl, c["i_node"], c["neg_samples"], c["seq_d1"], c["seq_d2"], c["label"], c["domain_id"])
                                  for c in batches])
            torch.cuda.synchronize()

        def run_fused(n):            # n batches: one device copy in, one graph replay, one device copy out, each
            for _ in range(n // NB):
                eng.eval_epoch(pl, packed, FIX, with_loss=True, use_graph=True)

        @torch.no_grad()
        def run_forward(n):          # the loop of train_sr.test() for a shape eval_ranks does not take
            keep = []
            for i in range(n):
                c = batches[i % NB]
                outs = model(None, c["i_node"], c["neg_samples"], c["seq_d1"], c["seq_d2"], None, None, False)
                p1, p2 = outs[0].reshape(B, -1), outs[1].reshape(B, -1)
                m2 = c["domain_id"].float().unsqueeze(1)
                keep.append((bce(p1, c["label"], reduction="none") * (1 - m2) + bce(p2, c["label"], reduction="none") * m2).mean())
                keep.append(device_positive_ranks(p1, p2, c["domain_id"], FIX))
            return keep

        def timed(fn, stream, n):
            fn(args.warmup // NB * NB + NB)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn(n)
            e1.record(stream)
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / n

        n = (args.reps + NB - 1) // NB * NB
        res = {"T": T, "B": B, "NI": NI, "batches_per_window": n, "fused_ok": bool(fused_ok)}
        fwd, fus = [], []
        for _ in range(2):
            fwd.append(round(timed(run_forward, torch.cuda.current_stream(), n), 4))
            if fused_ok:
                fus.append(round(timed(run_fused, eng.stream, n), 4))
        res["forward_loop_ms_per_batch"] = fwd
        res["fused_ms_per_batch"] = fus
        print(json.dumps(res), flush=True)
        del model, eng, pl, packed, batches
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
