"""Time the reference's own training loop on SASRec with torch.optim.Adam, with amid_amd.optim.Adam, and the fused train_step().

    python profiles/tools/reference_loop_time.py [--batches 8] [--windows 5] [--min_s 0.5] [--only loop_amid_adam]

SASRec, B 256 / T 50 / D 128 / hid 32, the reference-sized table of 894 820 rows, random weights; left-padded sequences of 1 .. T ids
drawn uniformly from the table, one negative a row; the reference's masked BCE (train_sr.py:203-212) written in torch.  Three
configurations, each on a model of its own, alternating window by window:
  * loop_torch_adam:  forward; optimizer.zero_grad(); loss.backward(); optimizer.step() with torch.optim.Adam -- the table's gradient is
                      materialised densely and Adam sweeps every parameter
  * loop_amid_adam:   the same loop with amid_amd.optim.Adam -- the table's gradient stays the step's unique rows, one optimizer launch
  * train_step:       model.train_step(): the whole step as one graph replay
A window repeats its configuration's --batches batches until --min_s has passed and ends in a device synchronise (host clock,
time.perf_counter); printed: ms per step of every window, median, spread (max - min).  For the two loops also the peak of
torch.cuda.max_memory_allocated over one step after the warm-up: absolute, and above what was allocated when the step began.
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
from amid_amd.optim import Adam  # noqa: E402

N_ROWS, D, HID, B, T = 894820, 128, 32, 256, 50


def batches(n, seed, dev):
    g = torch.Generator().manual_seed(seed)
    pad = N_ROWS - 1

    def seq():
        ids = torch.randint(1, pad, (n, B, T), generator=g)
        n_pad = torch.randint(0, T, (n, B, 1), generator=g)
        return torch.where(torch.arange(T) < n_pad, torch.full_like(ids, pad), ids)

    label = torch.zeros(B, 2)
    label[:, 0] = 1.0
    ep = dict(i_node=torch.randint(1, pad, (n, B), generator=g), neg_samples=torch.randint(1, pad, (n, B, 1), generator=g), seq_d1=seq(),
              seq_d2=seq(), domain_id=torch.randint(0, 2, (n, B), generator=g))
    ep = {k: v.to(dev) for k, v in ep.items()}
    return [dict({k: v[i] for k, v in ep.items()}, label=label.to(dev)) for i in range(n)]


def loop_step(model, optimizer, criterion, b):
    predict_d1, predict_d2 = model(None, b["i_node"], b["neg_samples"], b["seq_d1"], b["seq_d2"], None, None)
    mask_d1 = (1 - b["domain_id"]).unsqueeze(1)
    mask_d2 = b["domain_id"].unsqueeze(1)
    loss = torch.mean(criterion(predict_d1, b["label"]) * mask_d1 + criterion(predict_d2, b["label"]) * mask_d2)
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--min_s", type=float, default=0.5)
    ap.add_argument("--only", type=str, default="", help="one configuration (loop_torch_adam, loop_amid_adam, train_step)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    bs = batches(args.batches, 7, dev)
    criterion = torch.nn.BCELoss(reduction="none")
    make = lambda: SASRec(10, D, N_ROWS, D, T, HID, B, False, False, 0.5, 0.5, lr=5e-4, seed=1).cuda().train()      # noqa: E731
    configs, steps = {}, {}

    def add(name, one):
        if args.only and args.only != name:
            return
        steps[name] = one

        def run(one=one):
            for b in bs:
                one(b)
        configs[name] = run

    if not args.only or args.only == "loop_torch_adam":
        m_a = make()
        o_a = torch.optim.Adam(m_a.parameters(), lr=5e-4)
        add("loop_torch_adam", lambda b: loop_step(m_a, o_a, criterion, b))
    if not args.only or args.only == "loop_amid_adam":
        m_b = make()
        o_b = Adam(m_b.parameters(), lr=5e-4)
        add("loop_amid_adam", lambda b: loop_step(m_b, o_b, criterion, b))
    if not args.only or args.only == "train_step":
        m_c = make()
        add("train_step", lambda b: m_c.train_step(b["i_node"], b["neg_samples"], b["seq_d1"], b["seq_d2"], b["label"], b["domain_id"]))
    for fn in configs.values():                      # warm-up of every configuration (plans, optimizer state, the captured graph)
        fn()
    torch.cuda.synchronize()
    mem = {}
    for c in ("loop_torch_adam", "loop_amid_adam"):
        if c in steps:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            steps[c](bs[0])
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated()
            mem[c] = dict(peak_MiB=round(peak / 2 ** 20, 1), above_step_start_MiB=round((peak - base) / 2 ** 20, 1))
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
            ms[c].append(dt * 1e3 / (reps * len(bs)))
    for c, w in ms.items():
        print(json.dumps({"config": c, "B": B, "T": T, "D": D, "rows": N_ROWS, "batches": len(bs),
                          "clock": "host perf_counter around synchronised windows", "ms": [round(x, 4) for x in w],
                          "median": round(statistics.median(w), 4), "spread": round(max(w) - min(w), 4), **mem.get(c, {})}), flush=True)


if __name__ == "__main__":
    main()
