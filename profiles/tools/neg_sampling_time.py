"""Time the popularity-weighted negative sampler (csrc/sampling.hip, amid_sample_negatives_weighted_i64) against the uniform one
(amid_sample_negatives_i64) in the same process, on the same rows.

    python profiles/tools/neg_sampling_time.py [--launches 30] [--ks 1,999] [--powers 1.0,0.75]
    python profiles/tools/neg_sampling_time.py --rounds [--rounds_rows 512]        (needs no GPU)

Rows, pools and own lists: tests/golden/tok_cloth_sport_train75.npz through DualDomainSeqDataset.from_tokenised (15 403 rows, pools of
16 084 and 12 153 ids, counts from item_counts of the same dataset).  Configurations: uniform, and weighted at every power of --powers,
each at every k of --ks.  Timed with HIP events on one stream: three warm-up launches of every configuration, then --launches rounds
that alternate between the configurations, one launch bracketed by two events each; the epoch word advances every round, so no two
launches draw the same table.  Printed per configuration: median, minimum and maximum ms of a launch, the ratio of the medians to the
uniform kernel's at the same k, and the number of rows that fell short (none expected).
--rounds: the rounds histogram of the host restatement (tests/sampler_weighted_ref.py) at k = max(--ks) over --rounds_rows evenly spaced
rows, per power -- how many rounds of 64 candidates a row consumed; 16 is the floor for k = 999.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from amid_amd.dataset_seq import DualDomainSeqDataset, item_counts, popularity_weights  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "tok_cloth_sport_train75.npz")


def host_arrays(ds):
    off = np.zeros(len(ds) + 1, dtype=np.int32)
    np.cumsum([len(o) for o in ds.own_items], out=off[1:])
    return np.concatenate(ds.own_items), off


def rounds_of_row(ds, cums, r, k, seed=0, epoch=1):
    """Rounds of 64 candidates the restatement's row r consumes to keep k (4096: it fell short).  A row's stream depends on its index
    alone, so it is walked here without its neighbours."""
    from tests.sampler_weighted_ref import weighted_candidates
    dom = int(ds.domain_id[r] != 0)
    seen, n = set(ds.own_items[r].tolist()), 0
    for rnd in range(4096):
        for v in weighted_candidates(ds.pool[dom], cums[dom], r, rnd, 1, seed, epoch).tolist():
            if v not in seen:
                seen.add(v)
                n += 1
                if n == k:
                    return rnd + 1
    return 4096


def rounds_histogram(ds, counts, powers, k, n_rows):
    rows = np.unique(np.linspace(0, len(ds) - 1, n_rows).astype(np.int64))
    for power in powers:
        cums = [popularity_weights(c, power)[1] for c in counts]
        hist = {}
        for r in rows.tolist():
            used = rounds_of_row(ds, cums, r, k)
            hist[used] = hist.get(used, 0) + 1
        print(json.dumps({"power": power, "k": k, "rows": len(rows), "rounds_histogram": dict(sorted(hist.items())), "max": max(hist)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=30, help="timed launches of every configuration (>= 20)")
    ap.add_argument("--ks", type=str, default="1,999")
    ap.add_argument("--powers", type=str, default="1.0,0.75")
    ap.add_argument("--rounds", action="store_true", help="print the restatement's rounds histogram instead (CPU only)")
    ap.add_argument("--rounds_rows", type=int, default=512)
    args = ap.parse_args()
    ks, powers = [int(x) for x in args.ks.split(",")], [float(x) for x in args.powers.split(",")]
    ds = DualDomainSeqDataset.from_tokenised(FIXTURE)
    counts = item_counts(ds)
    if args.rounds:
        return rounds_histogram(ds, counts, powers, max(ks), args.rounds_rows)
    assert args.launches >= 20, "the median of at least 20 launches"
    assert torch.cuda.is_available(), "a timing needs the GPU"
    from amid_amd._lib import lib
    L, dev = lib(), torch.device("cuda:0")
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)       # noqa: E731
    own, off = host_arrays(ds)
    pool, d_own, d_off, d_dom = [to(p) for p in ds.pool], to(own), to(off), to(ds.domain_id)
    N, stream = len(ds), torch.cuda.current_stream().cuda_stream
    cums = {p: [popularity_weights(c, p)[1] for c in counts] for p in powers}
    d_cums = {p: [to(c) for c in cums[p]] for p in powers}
    for k in ks:
        out = torch.zeros(N, k, dtype=torch.int64, device=dev)

        def uniform(epoch):
            L.call("amid_sample_negatives_i64", pool[0].data_ptr(), pool[0].numel(), pool[1].data_ptr(), pool[1].numel(), d_own.data_ptr(),
                   d_off.data_ptr(), d_dom.data_ptr(), N, k, 0, epoch, out.data_ptr(), stream)

        def weighted(p):
            def run(epoch):
                L.call("amid_sample_negatives_weighted_i64", pool[0].data_ptr(), d_cums[p][0].data_ptr(), pool[0].numel(), pool[1].data_ptr(),
                       d_cums[p][1].data_ptr(), pool[1].numel(), int(cums[p][0][-1]), int(cums[p][1][-1]), d_own.data_ptr(), d_off.data_ptr(),
                       d_dom.data_ptr(), N, k, 0, epoch, out.data_ptr(), stream)
            return run

        configs = {"uniform": uniform, **{f"weighted_p{p}": weighted(p) for p in powers}}
        for c, fn in configs.items():
            for e in range(3):
                fn(1000 + e)
        torch.cuda.synchronize()
        ms, short = {c: [] for c in configs}, {c: 0 for c in configs}
        for i in range(args.launches):
            for c, fn in configs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(1 + i)
                e1.record()
                e1.synchronize()
                ms[c].append(e0.elapsed_time(e1))
                short[c] += int((out[:, 0] < 0).sum())
        base = statistics.median(ms["uniform"])
        for c in configs:
            w = ms[c]
            print(json.dumps({"config": c, "k": k, "rows": N, "launches": len(w), "median_ms": round(statistics.median(w), 4),
                              "min_ms": round(min(w), 4), "max_ms": round(max(w), 4), "ratio_to_uniform": round(statistics.median(w) / base, 2),
                              "short_rows": short[c]}), flush=True)


if __name__ == "__main__":
    main()
