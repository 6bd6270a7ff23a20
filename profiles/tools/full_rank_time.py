"""Time the full-catalog launches (amid_full_rank_f32, amid_topk_f32) with HIP events.

    python profiles/tools/full_rank_time.py [--reps 20] [--k 10]

Two shapes, B 256 users, D 128, hid 32, random weights and user vectors:
  * cloth_sport: the two item pools of tests/golden/tok_cloth_sport_train75.npz (every row of the table the reference's negatives
    can come from), a user's own items excluded (the fixture's own sets)
  * whole table: all 894 820 rows for every user
Prints per shape: us per batch of 256 users, table GB/s (the candidate rows read once per launch), scored (user, candidate) pairs/s.
Kernel-level splits: run it under `rocprofv3 --kernel-trace --stats -- python profiles/tools/full_rank_time.py --reps 5`.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from amid_amd._lib import lib  # noqa: E402

N_ROWS, D, HID, B = 894820, 128, 32, 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--k", type=int, default=10)
    args = ap.parse_args()
    L = lib()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    table = torch.randn(N_ROWS, D, generator=g).to(dev)
    a1 = 1.0 / (2 * D) ** 0.5
    w1 = ((torch.rand(HID, 2 * D, generator=g) * 2 - 1) * a1).to(dev)
    b1 = ((torch.rand(HID, generator=g) * 2 - 1) * a1).to(dev)
    w2 = ((torch.rand(1, HID, generator=g) * 2 - 1) / HID ** 0.5).to(dev)
    b2 = torch.zeros(1, device=dev)
    u = (torch.randn(B, D, generator=g) * 0.5).to(dev)
    dom = torch.randint(0, 2, (B,), generator=g).to(dev)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream

    z = np.load(os.path.join(ROOT, "tests", "golden", "tok_cloth_sport_train75.npz"))
    own_np, off_np = z["own"].astype(np.int64), z["own_off"].astype(np.int32)
    n_fix = len(off_np) - 1
    rows = torch.from_numpy(np.arange(B) % n_fix).to(torch.int32).to(dev)
    pos = torch.from_numpy(own_np[off_np[np.arange(B) % n_fix]]).to(dev)
    shapes = {
        "cloth_sport": (torch.from_numpy(z["pool_d1"].astype(np.int64)).to(dev), torch.from_numpy(z["pool_d2"].astype(np.int64)).to(dev),
                        torch.from_numpy(own_np).to(dev), torch.from_numpy(off_np).to(dev)),
        "whole_table": (torch.arange(N_ROWS, device=dev), torch.arange(N_ROWS, device=dev), None, None),
    }
    out = {}
    for name, (p1, p2, own, off) in shapes.items():
        n1, n2 = p1.numel(), p2.numel()
        ws = torch.empty(L.value("amid_full_rank_workspace_bytes", B, n1, n2, HID, args.k), dtype=torch.uint8, device=dev)
        rank = torch.empty(B, dtype=torch.int32, device=dev)
        raw = torch.empty_like(rank)
        ids = torch.empty(B, args.k, dtype=torch.int64, device=dev)
        sc = torch.empty(B, args.k, device=dev)
        ptr = lambda t: None if t is None else t.data_ptr()       # noqa: E731
        w = (table.data_ptr(), N_ROWS, w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), D, HID)

        def run_rank():
            L.call("amid_full_rank_f32", u.data_ptr(), 0, pos.data_ptr(), dom.data_ptr(), B, p1.data_ptr(), n1, p2.data_ptr(), n2, ptr(own),
                   ptr(off), ptr(rows) if own is not None else None, *w, 1e-7, ws.data_ptr(), flags.data_ptr(), rank.data_ptr(), raw.data_ptr(),
                   None, 0, s)

        def run_topk():
            L.call("amid_topk_f32", u.data_ptr(), 0, dom.data_ptr(), B, p1.data_ptr(), n1, p2.data_ptr(), n2, ptr(own), ptr(off),
                   ptr(rows) if own is not None else None, *w, args.k, 1, ws.data_ptr(), flags.data_ptr(), ids.data_ptr(), sc.data_ptr(), s)

        # pairs scored: every user against its own domain's pool
        n_dom1 = int(dom.sum())
        pairs = (B - n_dom1) * n1 + n_dom1 * n2
        gbytes = (n1 + n2) * D * 4 / 1e9
        res = {}
        for what, fn in (("rank", run_rank), ("topk", run_topk)):
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / args.reps
            res[what] = dict(us_per_batch=round(us, 1), table_GBps=round(gbytes / (us * 1e-6), 1), pairs_per_s=float(f"{pairs / (us * 1e-6):.4g}"))
        assert int(flags.item()) == 0
        out[name] = dict(B=B, n_pool=[n1, n2], pairs=pairs, k=args.k, **res)
        print(json.dumps({name: out[name]}), flush=True)


if __name__ == "__main__":
    main()
