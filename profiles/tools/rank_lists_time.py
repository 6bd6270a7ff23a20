"""Time the ranking of each row's own candidate list (csrc/rank_lists.hip) against a torch restatement on the same GPU, the same inputs, fp32.

    python profiles/tools/rank_lists_time.py [--windows 5] [--min_s 0.3] [--k 10] [--ours_only] [--cases test,skewed,many]

SASRec, D 128, hid 32, random weights, a table of 447 412 rows (the reference's item_length); synthetic N(0, 1) vectors in two domains;
candidate ids drawn uniformly from the table.  Three cases:
  * test     256 rows x 1 000 candidates each (test()'s shape)
  * skewed   256 rows, 256 000 candidates in all, ONE list holding half of them and the rest spread evenly over the other 255
  * many     4 096 rows x 100 candidates
Each as SASRec.rank_candidates_from_vectors with list_scores only (k=None) and with the top-K (k = --k, no list_scores), beside a torch
restatement: the lists padded to the longest one ([B, Lmax] index gather of the table -- the skewed case in chunks of rows so that the
padded block stays under 2 GB), the two half products as matmuls, add / relu / dot with w2 / sigmoid, and for the top-K a masked `topk`.
Timed, each with a warm-up, in --windows windows that alternate between the configurations; a window repeats its call until --min_s has
passed and ends in ONE device synchronise (host clock).  Printed per configuration: ms per call of every window, median, spread
(max - min), candidates per second, and the gathered bytes per second (candidates x D x 4) as a share of the 8.0 TB/s HBM peak.
Kernel-level split: `rocprofv3 --kernel-trace --stats -- python profiles/tools/rank_lists_time.py --windows 1 --min_s 0.05 --ours_only`.
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

from amid_amd.model_seq import SASRec  # noqa: E402

N_ROWS, D, HID, T = 447412, 128, 32, 50
HBM_PEAK = 8.0e12
PAD_BYTES = 2 << 30


def case_lengths(name):
    if name == "test":
        return [1000] * 256
    if name == "skewed":
        rest = 128000 // 255
        return [128000] + [rest + (1 if i < 128000 - rest * 255 else 0) for i in range(255)]
    if name == "many":
        return [100] * 4096
    raise SystemExit(f"unknown case {name!r} (test | skewed | many)")


def torch_rank(sd, V, items, off, lens, k):
    """list_scores [n] (k None) or (ids, scores, positions) [B, k]: the restatement in torch ops."""
    W1, b1 = sd["predictModule.fc.0.weight"], sd["predictModule.fc.0.bias"]
    w2, b2 = sd["predictModule.fc.2.weight"].reshape(-1), sd["predictModule.fc.2.bias"]
    table = sd["item_emb_layer.emb_item.weight"]
    B, dev = V.shape[0], V.device
    uh = V @ W1[:, :D].t() + b1                                          # [B, hid]
    lmax = int(lens.max())
    rows_at_once = max(1, min(B, PAD_BYTES // (lmax * D * 4)))
    out_ls = torch.empty(items.numel(), device=dev) if k is None else None
    outs = []
    for r0 in range(0, B, rows_at_once):
        r1 = min(B, r0 + rows_at_once)
        lm = int(lens[r0:r1].max())
        col = torch.arange(lm, device=dev)[None, :]
        live = col < lens[r0:r1, None]                                   # [b, lm]
        at = torch.where(live, off[r0:r1, None] + col, torch.zeros((), dtype=torch.int64, device=dev))
        ids = items[at]                                                  # padded index gather
        ih = table[ids] @ W1[:, D:].t()                                  # [b, lm, hid]
        p = torch.sigmoid(torch.relu(uh[r0:r1, None, :] + ih) @ w2 + b2)
        if k is None:
            out_ls[at[live]] = p[live]
        else:
            s, j = torch.where(live, p, torch.full((), float("-inf"), device=dev)).topk(min(k, lm), dim=1)
            outs.append((torch.gather(ids, 1, j), s, j))
    if k is None:
        return out_ls
    return tuple(torch.cat([o[i] for o in outs]) for i in range(3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--min_s", type=float, default=0.3)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--cases", type=str, default="test,skewed,many")
    ap.add_argument("--ours_only", action="store_true", help="for a profiler run: no torch restatement")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    model = SASRec(10, D, N_ROWS - 2, D, T, HID, 256, False, False, 0.5, 0.5, seed=1)
    model.eval()
    sd = {name: v.detach() for name, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(0)
    for name in args.cases.split(","):
        lens_h = torch.tensor(case_lengths(name), dtype=torch.int64)
        B, n = lens_h.numel(), int(lens_h.sum())
        off_h = torch.zeros(B + 1, dtype=torch.int64)
        off_h[1:] = torch.cumsum(lens_h, 0)
        V = torch.randn(B, D, generator=g).to(dev).contiguous()
        dom = torch.randint(0, 2, (B,), generator=g).to(dev)
        items = torch.randint(1, model.engine.n_rows - 1, (n,), generator=g).to(dev)
        off, lens = off_h.to(dev), lens_h.to(dev)
        cand = (items, off_h)
        configs = {"list_scores": lambda: model.rank_candidates_from_vectors(V, dom, cand, k=None, list_scores=True),
                   "top-K": lambda: model.rank_candidates_from_vectors(V, dom, cand, k=args.k)}
        if not args.ours_only:
            configs["torch list_scores"] = lambda: torch_rank(sd, V, items, off, lens, None)
            configs["torch top-K"] = lambda: torch_rank(sd, V, items, off, lens, args.k)
        res = {}
        for c, fn in configs.items():                                   # warm-up of every configuration
            res[c] = fn()
            torch.cuda.synchronize()
        agree = {}
        if not args.ours_only:
            agree["list_scores"] = float((res["list_scores"].list_scores - res["torch list_scores"]).abs().max())
            agree["top-K"] = float((res["top-K"].ids == res["torch top-K"][0]).float().mean())
        ms = {c: [] for c in configs}
        for _ in range(args.windows):
            for c, fn in configs.items():
                torch.cuda.synchronize()
                t0, reps = time.perf_counter(), 0
                while True:
                    for _ in range(4):
                        fn()
                    reps += 4
                    if time.perf_counter() - t0 >= args.min_s:
                        break
                torch.cuda.synchronize()
                ms[c].append((time.perf_counter() - t0) * 1e3 / reps)
        for c in configs:
            w = ms[c]
            med = statistics.median(w)
            out = {"case": name, "config": c, "B": B, "n_cand": n, "longest": int(lens_h.max()), "k": args.k, "D": D, "hid": HID,
                   "ms_per_call": [round(x, 4) for x in w], "median": round(med, 4), "spread": round(max(w) - min(w), 4),
                   "candidates_per_s": round(n / (med * 1e-3), 1), "gather_share_of_hbm_peak": round(n * D * 4 / (med * 1e-3) / HBM_PEAK, 4)}
            if c == "list_scores" and agree:
                out["max_abs_difference_vs_torch"] = agree["list_scores"]
            if c == "top-K" and agree:
                out["same_ids_share_vs_torch"] = agree["top-K"]
            print(json.dumps(out), flush=True)
        del res


if __name__ == "__main__":
    main()
