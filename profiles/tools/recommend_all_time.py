"""Time top-K over a dataset: SASRec.recommend_all (one graph replay a batch, item halves once) against a loop of SASRec.recommend().

    python profiles/tools/recommend_all_time.py [--batches 16] [--windows 5] [--min_s 0.5] [--k 10]

SASRec, D 128, hid 32, seq_len 50, the reference-sized table of 894 820 rows, random weights; B 256 users a batch, their sequences drawn
from the item pools of tests/golden/tok_cloth_sport_train75.npz (left-padded, 1 .. 50 ids long).  Two candidate sets:
  * cloth_sport: the fixture's two pools
  * table:       pool=None, every row of the table for every user
Three configurations, alternating window by window: the recommend() loop (unchanged by recommend_all's arrival: the same launches and
host-side set construction as before it), recommend_all with graphs, recommend_all eagerly.  A window repeats the whole set of batches until
--min_s has passed and ends in a device synchronise (host clock); printed: ms per batch of every window, median, spread (max - min), and
whether the three configurations returned the same ids and scores.
Kernel-level splits: run it under `rocprofv3 --kernel-trace --stats -- python profiles/tools/recommend_all_time.py --windows 1 --min_s 0.05`.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from amid_amd.model_seq import SASRec  # noqa: E402

N_ROWS, D, HID, B, T = 894820, 128, 32, 256, 50


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--min_s", type=float, default=0.5)
    ap.add_argument("--k", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    z = np.load(os.path.join(ROOT, "tests", "golden", "tok_cloth_sport_train75.npz"))
    pools_np = [z["pool_d1"].astype(np.int64), z["pool_d2"].astype(np.int64)]
    pad = int(z["pad_id"])
    rng = np.random.default_rng(0)
    n = args.batches
    seqs = np.full((2, n, B, T), pad, dtype=np.int64)
    for d in range(2):
        lens = rng.integers(1, T + 1, (n, B))
        draw = pools_np[d][rng.integers(0, len(pools_np[d]), (n, B, T))]
        keep = np.arange(T)[None, None, :] >= (T - lens)[:, :, None]
        seqs[d][keep] = draw[keep]
    users = {"seq_d1": torch.from_numpy(seqs[0]).to(dev), "seq_d2": torch.from_numpy(seqs[1]).to(dev),
             "domain_id": torch.from_numpy(rng.integers(0, 2, (n, B))).to(dev)}
    model = SASRec(10, D, N_ROWS, D, T, HID, B, False, False, 0.5, 0.5, seed=1)
    model.eval()
    pools = {"cloth_sport": tuple(torch.from_numpy(p).to(dev) for p in pools_np), "table": None}

    def loop(pool):
        outs = [model.recommend(users["seq_d1"][i], users["seq_d2"][i], users["domain_id"][i], k=args.k, pool=pool) for i in range(n)]
        return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])

    for name, pool in pools.items():
        configs = {"recommend() loop": lambda: loop(pool),
                   "recommend_all, graph": lambda: model.recommend_all(users, k=args.k, pool=pool, use_graph=True),
                   "recommend_all, eager": lambda: model.recommend_all(users, k=args.k, pool=pool, use_graph=False)}
        res = {c: fn() for c, fn in configs.items()}                     # warm-up of every configuration (captures the graph)
        torch.cuda.synchronize()
        ref = res["recommend() loop"]
        same = all(torch.equal(r[0], ref[0]) and torch.equal(r[1], ref[1]) for r in res.values())
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
        n_pool = [N_ROWS, N_ROWS] if pool is None else [int(p.numel()) for p in pool]
        for c in configs:
            w = ms[c]
            print(json.dumps({"pool": name, "n_pool": n_pool, "B": B, "T": T, "k": args.k, "batches": n, "config": c,
                              "ms_per_batch": [round(x, 5) for x in w], "median": round(statistics.median(w), 5),
                              "spread": round(max(w) - min(w), 5), "same_results": same}), flush=True)


if __name__ == "__main__":
    main()
