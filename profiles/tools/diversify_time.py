"""Time the diversified top-K (csrc/diversify.hip, amid_mmr_lists_f32) against a torch restatement on the same GPU, the same inputs, fp32.

    python profiles/tools/diversify_time.py [--windows 5] [--min_s 0.5] [--metric cosine] [--lam 0.7] [--ours_only] [--cases short,full]

A randn table of 447 412 rows x D 128 (the reference's item_length), distinct ids drawn from it for every list, uniform relevances.  Cases:
  * short   256 rows x lists of 1 000 -> shortlist 100 -> k 10
  * full    256 rows x lists of 256   -> shortlist 256 -> k 256
Ours: the three launches of amid_mmr_lists_f32 captured once into a graph and replayed.  The torch restatement, also captured and
replayed: topk of the relevance for the shortlist, one gather of the shortlist's table rows [B, M, D], the M x M similarity block by bmm
(rows normalised for the cosine), then k greedy rounds of maximum / multiply-subtract / masked argmax over [B, M] -- what a host-side
implementation does; it has no rule for repeated ids and ties go where argmax sends them (the inputs here have neither).
Timed, each after a warm-up, in --windows windows that alternate between the two; a window replays its graph until --min_s has passed
and ends in ONE device synchronise (host clock).  Printed per configuration: ms per call of every window, median, spread (max - min), and
the share of rows on which the two agree on every pick.
Kernel-level split: `rocprofv3 --kernel-trace --stats -- python profiles/tools/diversify_time.py --windows 1 --min_s 0.05 --ours_only`.
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

from amid_amd._lib import lib  # noqa: E402

N_ROWS, D = 447412, 128
CASES = {"short": (256, 1000, 100, 10), "full": (256, 256, 256, 256)}      # rows, list length, shortlist, k


def torch_mmr(table, items, rel, M, K, metric, lam, out_ids):
    """items / rel [B, L] -> out_ids [B, K]."""
    B = items.shape[0]
    r, at = rel.topk(M, dim=1)                                           # the shortlist, best first
    ids = torch.gather(items, 1, at)
    X = table[ids]                                                       # [B, M, D]
    if metric == 1:
        X = X / X.norm(dim=2, keepdim=True).clamp(min=1e-8)
    S = torch.bmm(X, X.transpose(1, 2))                                  # [B, M, M]
    lr, oml = lam * r, 1.0 - lam
    taken = torch.zeros(B, M, dtype=torch.bool, device=items.device)
    m = torch.full((B, M), float("-inf"), device=items.device)
    p = torch.zeros(B, 1, dtype=torch.int64, device=items.device)
    for j in range(K):                                                   # (gather / scatter only: indexed assignment cannot be captured)
        if j > 0:
            v = (lr - oml * m).masked_fill(taken, float("-inf"))
            p = v.argmax(dim=1, keepdim=True)
        out_ids[:, j:j + 1] = torch.gather(ids, 1, p)
        taken = taken.scatter(1, p, True)
        m = torch.maximum(m, torch.gather(S, 2, p[:, :, None].expand(B, M, 1)).squeeze(2))
    return out_ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--min_s", type=float, default=0.5)
    ap.add_argument("--metric", type=str, default="cosine", choices=("cosine", "dot"))
    ap.add_argument("--lam", type=float, default=0.7)
    ap.add_argument("--cases", type=str, default="short,full")
    ap.add_argument("--ours_only", action="store_true", help="for a profiler run: no torch restatement")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    metric = 1 if args.metric == "cosine" else 0
    g = torch.Generator().manual_seed(0)
    table = torch.randn(N_ROWS, D, generator=g).to(dev)
    L = lib()
    for name in args.cases.split(","):
        B, n_list, M, K = CASES[name]
        items = torch.stack([torch.randperm(N_ROWS, generator=g)[:n_list] for _ in range(B)]).to(dev)
        rel = torch.rand(B, n_list, generator=g).to(dev)
        off = (torch.arange(B + 1, dtype=torch.int64) * n_list).to(dev)
        n = B * n_list
        ws = torch.empty(int(L.value("amid_mmr_workspace_bytes", B, n, D, K, M)), dtype=torch.uint8, device=dev)
        flags = torch.zeros(1, dtype=torch.int32, device=dev)
        ids = torch.empty(B, K, dtype=torch.int64, device=dev)
        pos = torch.empty(B, K, dtype=torch.int64, device=dev)
        sc, val, ms_ = (torch.empty(B, K, device=dev) for _ in range(3))
        t_ids = torch.empty(B, K, dtype=torch.int64, device=dev)

        def ours():
            L.call("amid_mmr_lists_f32", items.data_ptr(), off.data_ptr(), rel.data_ptr(), n, B, table.data_ptr(), N_ROWS, D, metric, args.lam, K, M,
                   ws.data_ptr(), flags.data_ptr(), ids.data_ptr(), sc.data_ptr(), val.data_ptr(), ms_.data_ptr(), pos.data_ptr(),
                   torch.cuda.current_stream().cuda_stream)

        configs = {"ours": ours}
        if not args.ours_only:
            configs["torch"] = lambda: torch_mmr(table, items, rel, M, K, metric, args.lam, t_ids)
        graphs = {}
        side = torch.cuda.Stream()
        for c, fn in configs.items():                                    # warm-up on the side stream, then the capture
            with torch.cuda.stream(side):
                fn()
            torch.cuda.synchronize()
            graphs[c] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[c], stream=side):
                fn()
            graphs[c].replay()
            torch.cuda.synchronize()
        assert int(flags.item()) == 0
        same = None if args.ours_only else float((ids == t_ids).all(dim=1).float().mean())
        ms = {c: [] for c in configs}
        for _ in range(args.windows):
            for c in configs:
                torch.cuda.synchronize()
                t0, reps = time.perf_counter(), 0
                while True:
                    for _ in range(4):
                        graphs[c].replay()
                    reps += 4
                    if time.perf_counter() - t0 >= args.min_s:
                        break
                torch.cuda.synchronize()
                ms[c].append((time.perf_counter() - t0) * 1e3 / reps)
        for c in configs:
            w = ms[c]
            out = {"case": name, "config": c, "B": B, "list": n_list, "shortlist": M, "k": K, "D": D, "metric": args.metric, "lam": args.lam,
                   "ms_per_call": [round(x, 4) for x in w], "median": round(statistics.median(w), 4), "spread": round(max(w) - min(w), 4)}
            if same is not None:
                out["rows_with_the_same_picks_share"] = same
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
