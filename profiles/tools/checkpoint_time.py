"""Time a checkpoint of the full table: SASRec.save_training_state / load_training_state (device <-> host transfer + serialisation
to a file) and the HBM best-model snapshot of train_sr.py --save_dir (device-to-device copies of the table and the dense buffer).

    python profiles/tools/checkpoint_time.py [--dir DIR] [--reps 3]

SASRec with 894 820 rows x D 128, T 50, hid 32 (the CLI's table), its Adam state allocated; once plain, once with the doubly-robust
model's second Adam state (isDR, both states stepped).  One JSON line per case: file GB, seconds (best, median) of training_state()
(device -> host copies), torch.save, the whole save_training_state, load_training_state (file -> device, in place), and us per
best-model snapshot (HIP events).  The file goes to a temporary directory under DIR (default: the system's), removed at the end.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from amid_amd.model_seq import SASRec  # noqa: E402
from amid_amd.train_sr import BestModels  # noqa: E402

N_ROWS, D, T, HID = 894820, 128, 50, 32


def _best(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t)
    return round(min(out), 3), round(sorted(out)[len(out) // 2], 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default=None)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    root = tempfile.mkdtemp(dir=args.dir)
    try:
        for dr in (False, True):
            m = SASRec(10, D, N_ROWS, D, T, HID, 256, False, False, 0.5, 0.5, isDR=dr, seed=0)
            eng = m.engine
            eng._ensure_opt_state()
            if dr:
                eng.select_optimizer(1)
                eng._ensure_opt_state()
            eng.sync()
            path = os.path.join(root, "last.pt")
            res = {"case": "sasrec_dr_two_adam_states" if dr else "sasrec", "n_rows": N_ROWS, "D": D}
            res["training_state_s"] = _best(eng.training_state, args.reps)
            st = eng.training_state()
            res["torch_save_s"] = _best(lambda: torch.save({"format": 1, "engine": st, "extra": {}}, path), args.reps)
            del st
            res["save_training_state_s"] = _best(lambda: m.save_training_state(path), args.reps)
            res["file_GB"] = round(os.path.getsize(path) / 1e9, 3)
            res["load_training_state_s"] = _best(lambda: m.load_training_state(path), args.reps)
            bm = BestModels(m)
            bm.snapshot("d1")
            eng.sync()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            n = 20
            e0.record(eng.stream)
            for _ in range(n):
                bm.snapshot("d1")          # flush pass (no pending rows) + table and dense copies, on the engine's stream
            e1.record(eng.stream)
            e1.synchronize()
            res["hbm_snapshot_us"] = round(e0.elapsed_time(e1) * 1e3 / n, 1)
            res["hbm_snapshot_GBps"] = round(2 * (eng.table.numel() + eng.dense.data.numel()) * 4 / (res["hbm_snapshot_us"] * 1e3), 1)
            print(json.dumps(res), flush=True)
            del bm, m, eng
            torch.cuda.empty_cache()
            os.remove(path)
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
