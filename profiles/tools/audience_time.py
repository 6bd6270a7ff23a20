"""Time the audience top-K (csrc/audience.hip: "which users for this item") against a torch restatement on the same GPU, the same inputs, fp32.

    python profiles/tools/audience_time.py [--windows 5] [--min_s 0.5] [--n 895510] [--q 256] [--k 100] [--chunk 65536] [--ours_only]

SASRec, D 128, hid 32, random weights, a table of 447 412 rows; N = 895 510 synthetic N(0, 1) vectors (the reference's user_length) in two
domains drawn at random, Q = 256 distinct query items in two domains, k = 100, no holders.  Timed, each with a warm-up, in --windows windows
that alternate between the configurations; a window repeats its call until --min_s has passed and ends in ONE device synchronise (host
clock), so the launches of a window queue back to back:
  * halves         SasrecEngine.enqueue_audience_halves alone: N D 4 bytes read + N hid 4 written, as a share of the 8.0 TB/s HBM peak (and of
                   the 6.29 TB/s a float4 copy reaches, MI355X_MICROARCH.md)
  * top-K          SasrecEngine.enqueue_audience_topk alone (the queries' item halves, the per-range lists, the merge) on those halves
  * recommend_users  the whole call: slot lists, halves, top-K, the flag read
  * torch          the two half products (V W1[:, :D]^T + b1 once per call, E[items] W1[:, D:]^T), then per chunk of --chunk rows the broadcast
                   add / relu / dot with w2 / sigmoid of the chunk against the queries of its domain, `topk` per chunk, the chunks' winners
                   merged by a last `topk`
Printed per configuration: ms per call of every window, median, spread (max - min); and the share of (query, rank) slots where the two
sides name the same row.
Kernel-level split: `rocprofv3 --kernel-trace --stats -- python profiles/tools/audience_time.py --windows 1 --min_s 0.05 --ours_only`.
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
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12


def torch_audience(sd, V, vdom, items, item_dom, k, chunk):
    """rows [Q, k], scores [Q, k]: the restatement in torch ops (a row index -1 where a domain has fewer than k rows)."""
    W1, b1 = sd["predictModule.fc.0.weight"], sd["predictModule.fc.0.bias"]
    w2, b2 = sd["predictModule.fc.2.weight"].reshape(-1), sd["predictModule.fc.2.bias"]
    uh = V @ W1[:, :D].t() + b1                                         # [N, hid]
    ih = sd["item_emb_layer.emb_item.weight"][items] @ W1[:, D:].t()    # [Q, hid]
    Q = items.shape[0]
    rows = torch.full((Q, k), -1, dtype=torch.int64, device=V.device)
    scores = torch.full((Q, k), float("-inf"), device=V.device)
    for d in (0, 1):
        qs = torch.nonzero((item_dom != 0) == bool(d)).reshape(-1)
        rs = torch.nonzero((vdom != 0) == bool(d)).reshape(-1)
        if qs.numel() == 0 or rs.numel() == 0:
            continue
        best_s, best_i = [], []
        for c0 in range(0, rs.numel(), chunk):
            r = rs[c0:c0 + chunk]
            p = torch.sigmoid(torch.relu(uh[r][None, :, :] + ih[qs][:, None, :]) @ w2 + b2)       # [Qd, chunk]
            s, i = p.topk(min(k, r.numel()), dim=1)
            best_s.append(s)
            best_i.append(r[i])
        s, i = torch.cat(best_s, 1), torch.cat(best_i, 1)
        s, j = s.topk(min(k, s.shape[1]), dim=1)
        rows[qs, :s.shape[1]] = torch.gather(i, 1, j)
        scores[qs, :s.shape[1]] = s
    return rows, scores


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--min_s", type=float, default=0.5)
    ap.add_argument("--n", type=int, default=895510)
    ap.add_argument("--q", type=int, default=256)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--ours_only", action="store_true", help="for a profiler run: no torch restatement")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    dev = torch.device("cuda:0")
    model = SASRec(10, D, N_ROWS - 2, D, T, HID, 256, False, False, 0.5, 0.5, seed=1)
    model.eval()
    eng = model.engine
    g = torch.Generator().manual_seed(0)
    V = torch.randn(args.n, D, generator=g).to(dev).contiguous()
    vdom = torch.randint(0, 2, (args.n,), generator=g).to(dev)
    items = torch.randperm(min(eng.n_rows, 400000), generator=g)[:args.q].to(dev)
    item_dom = torch.randint(0, 2, (args.q,), generator=g).to(dev)
    sd = {name: v.detach() for name, v in model.state_dict().items()}
    slots = (torch.nonzero(vdom == 0).reshape(-1).to(torch.int32), torch.nonzero(vdom != 0).reshape(-1).to(torch.int32))
    rows = torch.empty(args.q, args.k, dtype=torch.int64, device=dev)
    scores = torch.empty(args.q, args.k, device=dev)
    err = eng.flags_holder().err
    torch.cuda.synchronize()

    def halves():
        eng.enqueue_audience_halves(V, slots)

    def topk():
        for c0 in range(0, args.q, eng.AUDIENCE_CHUNK):
            c1 = min(args.q, c0 + eng.AUDIENCE_CHUNK)
            eng.enqueue_audience_topk(items[c0:c1], item_dom[c0:c1], slots, None, args.k, rows[c0:c1], scores[c0:c1], err)

    configs = {"halves": halves, "top-K": topk, "recommend_users": lambda: model.recommend_users(items, item_dom, V, vdom, k=args.k)}
    if not args.ours_only:
        configs["torch"] = lambda: torch_audience(sd, V, vdom, items, item_dom, args.k, args.chunk)
    res = {}
    for c, fn in configs.items():                                       # warm-up of every configuration
        res[c] = fn()
        torch.cuda.synchronize()
    agree = None
    if not args.ours_only:
        agree = float((res["recommend_users"][0] == res["torch"][0]).float().mean())
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
        out = {"config": c, "N": args.n, "Q": args.q, "k": args.k, "D": D, "hid": HID, "ms_per_call": [round(x, 4) for x in w],
               "median": round(med, 4), "spread": round(max(w) - min(w), 4)}
        if c == "halves":
            nbytes = args.n * (D + HID) * 4
            out.update(bytes=nbytes, share_of_hbm_peak=round(nbytes / (med * 1e-3) / HBM_PEAK, 4),
                       share_of_float4_copy_rate=round(nbytes / (med * 1e-3) / HBM_COPY, 4))
        if c == "top-K":
            out["pairs_per_s"] = round(args.n / 2 * args.q / (med * 1e-3), 1)
        if c == "recommend_users":
            out["same_rows_share_vs_torch"] = agree
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
