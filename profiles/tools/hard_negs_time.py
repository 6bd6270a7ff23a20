"""Time the hard-negative launch (csrc/head_mined.hip, amid_scorer_mined_fwd_bwd_f32) against the listwise launch it extends
(amid_scorer_listwise_fwd_bwd_f32), and the train step with and without mining.

    python profiles/tools/hard_negs_time.py [--launches 200] [--rounds 7] [--kind 1] [--steps]

Launches: B 256, D 128, hid 32, randn inputs; for NI in 65 / 257 / 1024 and H in 4 / 16 / 64 (S 0), in one process on the same buffers,
alternated round by round after 20 warm-up launches each:
  * mined      the new launch at (NI, H)
  * full       the listwise launch at the same NI (every negative kept)
  * full_again the listwise launch at the same NI a second time: the A/A spread of that launch against itself in this run
  * short      the listwise launch at NI = 1 + H (what a loader that drew H negatives would run)
Each figure is the time between two HIP events around --launches launches, divided by their number; printed per configuration: every
round's us, the median, min and max.  The expectation checked by eye, not asserted: short <= mined <= full.

--steps: SASRec, B 256, T 50, D 128, hid 32, a table of 50 000 rows, an input pool of 8 batches, dropout on, one captured single-step graph
replayed per step; 16 warm-up steps, then 3 rounds of 200 steps under a host clock that ends in a stream synchronise, the models alternated:
--train_negs 256 --hard_negs 16, --train_negs 256, --train_negs 16 (softmax)."""
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

B, D, HID = 256, 128, 32


def launch_times(args):
    L, dev = lib(), torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    s = torch.cuda.current_stream().cuda_stream
    w = dict(w1=(torch.randn(HID, 2 * D, generator=g) / (2 * D) ** 0.5), b1=0.1 * torch.randn(HID, generator=g),
             w2=torch.randn(HID, generator=g) / HID ** 0.5, b2=torch.zeros(1))
    w = {k: v.to(dev) for k, v in w.items()}
    u = torch.randn(2, B, D, generator=g).to(dev)
    dom = torch.randint(0, 2, (B,), generator=g).to(dev)
    P = int(L.value("amid_scorer_part_floats", D, HID))
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for NI in (65, 257, 1024):
        items = torch.randn(B, NI, D, generator=g).to(dev)
        f = lambda *shape: torch.empty(*shape, device=dev)      # noqa: E731
        o = dict(p1=f(B, NI), p2=f(B, NI), dz1=f(B, NI), dz2=f(B, NI), loss_part=f(B), du=f(2, B, D), ditems=f(B, NI, D), sc_part=f(B, P))
        z = f(B, NI)
        for H in (4, 16, 64):
            sel = torch.empty(B, H, dtype=torch.int32, device=dev)
            short_items = items[:, :1 + H].contiguous()
            base = dict({k: v.data_ptr() for k, v in w.items()}, u=u.data_ptr(), domain_id=dom.data_ptr(), kind=args.kind, B=B, D=D, hid=HID,
                        tr_src=None, tr_dst=None, n_tr=0, stream=s, **{k: v.data_ptr() for k, v in o.items()})
            full = lambda: L.call_named("amid_scorer_listwise_fwd_bwd_f32", base, items=items.data_ptr(), NI=NI)      # noqa: E731
            configs = {
                "mined": lambda: L.call_named("amid_scorer_mined_fwd_bwd_f32", base, items=items.data_ptr(), NI=NI, keep=H, skip=0,
                                              sel=sel.data_ptr(), z=z.data_ptr()),
                "full": full, "full_again": full,
                "short": lambda: L.call_named("amid_scorer_listwise_fwd_bwd_f32", base, items=short_items.data_ptr(), NI=1 + H),
            }
            us = {c: [] for c in configs}
            for fn in configs.values():
                for _ in range(20):
                    fn()
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for c, fn in configs.items():
                    ev0.record()
                    for _ in range(args.launches):
                        fn()
                    ev1.record()
                    ev1.synchronize()
                    us[c].append(ev0.elapsed_time(ev1) * 1e3 / args.launches)
            for c, v in us.items():
                print(json.dumps({"what": "launch", "config": c, "B": B, "NI": NI if c != "short" else 1 + H, "H": H, "D": D, "hid": HID, "kind": args.kind,
                                  "us": [round(x, 2) for x in v], "median": round(statistics.median(v), 2), "min": round(min(v), 2),
                                  "max": round(max(v), 2)}), flush=True)


def step_times(args):
    from amid_amd.model_seq import SASRec
    T, n_items, n_pool = 50, 50000, 8
    cfgs = {"negs256_hard16": (256, dict(hard_negs=16)), "negs256": (256, {}), "negs16": (16, {})}
    models = {}
    for name, (K, kw) in cfgs.items():
        g = torch.Generator().manual_seed(1)
        pad = n_items - 1
        ids = lambda *shape: torch.randint(1, pad, shape, generator=g)      # noqa: E731
        label = torch.zeros(B, 1 + K)
        label[:, 0] = 1.0
        ep = dict(i_node=ids(n_pool, B), neg_samples=ids(n_pool, B, K), seq_d1=ids(n_pool, B, T), seq_d2=ids(n_pool, B, T),
                  domain_id=torch.randint(0, 2, (n_pool, B), generator=g), label=label)
        m = SASRec(10, D, n_items, D, T, HID, B, False, False, 0.5, 0.5, lr=1e-3, seed=0, loss="softmax", **kw)
        m.train()
        m.begin_epoch_pool({k: v.cuda() for k, v in ep.items()})
        for _ in range(16):
            m.pool_step(use_graph=True)
        m.engine.sync()
        models[name] = m
    ms = {c: [] for c in models}
    for _ in range(3):
        for c, m in models.items():
            m.engine.sync()
            t0 = time.perf_counter()
            for _ in range(200):
                m.pool_step(use_graph=True)
            m.engine.sync()
            ms[c].append((time.perf_counter() - t0) * 1e3 / 200)
    for c, v in ms.items():
        print(json.dumps({"what": "step", "config": c, "B": B, "T": T, "D": D, "ms": [round(x, 4) for x in v], "median": round(statistics.median(v), 4),
                          "min": round(min(v), 4), "max": round(max(v), 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--kind", type=int, default=1, choices=(1, 2))
    ap.add_argument("--steps", action="store_true", help="the train-step comparison instead of the launches")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    (step_times if args.steps else launch_times)(args)


if __name__ == "__main__":
    main()
