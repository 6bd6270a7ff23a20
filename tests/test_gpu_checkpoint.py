"""Save and resume the fused training state (SasrecEngine.training_state / load_training_state, SASRec.save_training_state /
load_training_state, DeviceBatches.state_dict, train_sr.py / train_sr_dr.py --save_dir / --save_every / --resume): a run resumed
from a file is the uninterrupted run, bit for bit; the best-model files are the best epochs' weights."""
import itertools
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ITEMS, T, B = 400, 20, 16
HOT = (300, 340)           # ids that only the batches named by _epoch(hot=...) hold


def _epoch(n, seed, hot=()):
    """n batches laid out as DeviceBatches.epoch_tensors() lays them out; left-padded sequences, ids below HOT[0] except the
    positives of the batches in `hot`."""
    g = torch.Generator().manual_seed(seed)
    pad = N_ITEMS - 1

    def seq():
        ids = torch.randint(1, HOT[0], (n, B, T), generator=g)
        n_pad = torch.randint(0, T, (n, B, 1), generator=g)
        return torch.where(torch.arange(T) < n_pad, torch.full_like(ids, pad), ids)

    i_node = torch.randint(1, HOT[0], (n, B), generator=g)
    for i in hot:
        i_node[i] = torch.randint(*HOT, (B,), generator=g)
    label = torch.zeros(B, 2)
    label[:, 0] = 1.0
    ep = dict(i_node=i_node, neg_samples=torch.randint(1, HOT[0], (n, B, 1), generator=g), seq_d1=seq(), seq_d2=seq(),
              domain_id=torch.randint(0, 2, (n, B), generator=g), ob_label=torch.randint(0, 2, (n, B), generator=g), label=label)
    return {k: v.cuda() for k, v in ep.items()}


def _model(kind, seed):
    from amid_amd.model_seq import BERT4Rec, SASRec
    if kind == "bert4rec":
        return BERT4Rec(10, 128, N_ITEMS, 128, T, 16, B, False, False, 0.5, 0.5, lr=1e-3, seed=seed)
    D = 128 if kind == "bf16" else 64
    return SASRec(10, D, N_ITEMS, D, T, 16, B, kind == "inc", kind == "itc_dr", 0.02, 0.4, isDR=kind == "itc_dr", lr=1e-3, seed=seed,
                  compute="bf16" if kind == "bf16" else "f32")


def _host(x, eng):
    eng.sync()
    return x.detach().cpu().clone()


def _steps(m, ep, idx, use_graph=True, k=None):
    """train_step() over the batches idx of ep (k: the DR objective on Adam state k); returns the losses."""
    out = []
    for i in idx:
        loss = m.train_step(ep["i_node"][i], ep["neg_samples"][i], ep["seq_d1"][i], ep["seq_d2"][i], ep["label"], ep["domain_id"][i],
                            use_graph=use_graph, ob_label=ep["ob_label"][i] if k is not None else None, dr_objective=k or 0)
        out.append(_host(loss, m.engine))
    return out


def _train(m, kind, ep):
    """One epoch of ep the way `kind` trains; returns the losses the host sees."""
    eng, n = m.engine, ep["seq_d1"].shape[0]
    if kind in ("pool4", "pool_eager", "bf16"):
        m.begin_epoch_pool(ep)
        if kind == "pool_eager":
            out = [_host(m.pool_step(use_graph=False), eng) for _ in range(n)]
        else:
            out = [_host(m.pool_step(n_steps=4), eng) for _ in range(n // 4)]
        m.end_epoch_pool()
        return out
    if kind == "itc_dr":                 # run.sh's model: both objectives, each on its own Adam state (train_sr_dr.py)
        out = []
        for k, lr in ((0, 1e-3), (1, 5e-4)):
            eng.select_optimizer(k, lr=lr)
            out += _steps(m, ep, range(n), k=k)
        return out
    return _steps(m, ep, range(n))


def _flat(x, prefix=""):
    if isinstance(x, dict):
        out = {}
        for k, v in x.items():
            out.update(_flat(v, f"{prefix}/{k}"))
        return out
    return {prefix: x}


def _assert_same(a, b):
    fa, fb = _flat(a), _flat(b)
    assert fa.keys() == fb.keys()
    for k in fa:
        if isinstance(fa[k], torch.Tensor):
            assert fa[k].dtype == fb[k].dtype and torch.equal(fa[k], fb[k]), k
        else:
            assert fa[k] == fb[k], k


def _flushed_state(m):
    m.engine.flush_table()
    m.engine.sync()
    return m.engine.training_state()


def _resume_and_compare(path, kind, a, la, ep2, seed):
    b = _model(kind, seed)
    extra = b.load_training_state(path)
    lb = _train(b, kind, ep2)
    assert len(la) == len(lb) > 0
    for x, y in zip(la, lb):
        assert torch.equal(x, y)
    _assert_same(_flushed_state(a), _flushed_state(b))
    return extra


@pytest.mark.parametrize("kind", ["pool4", "pool_eager", "itc_dr", "inc", "bert4rec", "bf16"])
def test_resume_equals_uninterrupted(tmp_path, kind):
    e1, e2 = _epoch(8, 1), _epoch(8, 2)
    a = _model(kind, 3)
    _train(a, kind, e1)
    path = tmp_path / "a.pt"
    a.save_training_state(path, epoch=0, note="x")
    la = _train(a, kind, e2)
    st = torch.load(path, weights_only=True)["engine"]
    assert set(st["optimizer"]["banks"]) == ({0, 1} if kind == "itc_dr" else {0})
    assert st["optimizer"]["banks"][st["optimizer"]["opt_bank"]]["step"] == 8
    assert _resume_and_compare(path, kind, a, la, e2, 4) == {"epoch": 0, "note": "x"}


def test_pending_lazy_rows_cross_the_save(tmp_path):
    e1, e2 = _epoch(8, 5, hot=(0, 1)), _epoch(8, 6, hot=range(8))
    a = _model("pool4", 7)
    _train(a, "pool4", e1)
    path = tmp_path / "a.pt"
    a.save_training_state(path)
    bank = torch.load(path, weights_only=True)["engine"]["optimizer"]["banks"][0]
    tl, step = bank["table_last"][HOT[0]:HOT[1]].long(), bank["step"]
    # rows touched by the first two steps only: they owe >= 5 zero-gradient steps, and the file keeps them owing
    assert step == 8 and int(((tl > 0) & (tl <= step - 5)).sum()) > 0
    la = _train(a, "pool4", e2)
    _resume_and_compare(path, "pool4", a, la, e2, 8)


def test_captured_graph_survives_a_load(tmp_path):
    e = _epoch(6, 9)
    a = _model("graph", 10)
    _steps(a, e, range(3))
    path = tmp_path / "a.pt"
    a.save_training_state(path)
    m = _model("graph", 11)
    _steps(m, e, range(3, 6))                    # captures the step's graph over m's own buffers
    pl, key = m._last_plan, m.engine._graph_key()
    g0 = pl.graphs[key]
    m.load_training_state(path)
    assert pl.graphs.get(key) == g0
    lm = _steps(m, e, range(3, 6), use_graph=True)
    assert pl.graphs[key] == g0                  # replayed, not captured again
    r = _model("graph", 12)
    r.load_training_state(path)
    lr = _steps(r, e, range(3, 6), use_graph=False)
    for x, y in zip(lm, lr):
        assert torch.equal(x, y)
    _assert_same(_flushed_state(m), _flushed_state(r))


def test_refusals(tmp_path):
    from amid_amd.model_seq import BERT4Rec, SASRec

    def mk(D=64, isItC=False, **kw):
        return SASRec(10, D, N_ITEMS, D, T, 16, B, False, isItC, 0.5, 0.5, **kw)

    def saved(m, name):
        p = tmp_path / name
        m.save_training_state(p)
        return p

    p64, p128 = saved(mk(), "d64.pt"), saved(mk(128), "d128.pt")
    for other, field in ((mk(128), "D"), (mk(isDR=True), "dr"), (mk(isItC=True), "itc_bs")):
        with pytest.raises(ValueError, match=f": {field} is "):
            other.load_training_state(p64)
    with pytest.raises(ValueError, match=": compute is 'f32' in the state, 'bf16' here"):
        mk(128, compute="bf16").load_training_state(p128)
    pb = saved(BERT4Rec(10, 128, N_ITEMS, 128, T, 16, B, False, False, 0.5, 0.5), "bert.pt")
    with pytest.raises(ValueError, match=": engine is 'Bert4recEngine' in the state, 'SasrecEngine' here"):
        mk(128).load_training_state(pb)
    pooled = mk()
    pooled.begin_epoch_pool(_epoch(4, 1))
    with pytest.raises(ValueError, match="drop_epoch_pool"):
        pooled.load_training_state(p64)
    pooled.drop_epoch_pool()
    pooled.load_training_state(p64)


# ---------------------------------------------------------------------------------------------- the command line, in fresh processes
COMMON = ["--bs", "32", "--seq_len", "20", "--emb_dim", "64", "--hid_dim", "16", "--neg_nums", "19"]


def _data(tmp_path, dr):
    from tests.test_gpu_module import _write_csv
    rng = np.random.default_rng(11)
    if dr:
        root = tmp_path / "mybank_dataset"
        root.mkdir()
        _write_csv(root / "toy_train25.csv", 160, rng, 1, 300, 300, 700)
        _write_csv(root / "toy_train25_DR.csv", 130, rng, 1, 300, 300, 700, ob_label=True)
        _write_csv(root / "toy_test.csv", 64, rng, 1, 300, 300, 700)
        return ["--data_root", str(tmp_path), "-ds", "mybank", "-dm", "toy", "--overlap_ratio", "0.25", "--model", "sasrec",
                "--isItC", "True", "--ts2", "0.4", "--isDR", "True", "--lr2", "0.5", "--dr_e_w", "0.1"] + COMMON
    root = tmp_path / "amazon_dataset"
    root.mkdir()
    _write_csv(root / "toy_train75.csv", 300, rng, 1, 400, 400, 900)
    _write_csv(root / "toy_test.csv", 80, rng, 1, 400, 400, 900)
    return ["--data_root", str(tmp_path), "-ds", "amazon", "-dm", "toy", "--overlap_ratio", "0.75", "--model", "sasrec"] + COMMON


def _cli(mod, args):
    r = subprocess.run([sys.executable, "-m", mod] + args, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]


def _log(path):
    return [re.sub(r"^\[[0-9/:,. -]+\] ", "", line) for line in path.read_text().splitlines()]      # (timestamps dropped)


def _seed0_epoch1(path, n_epochs):
    """Seed 0's epoch 1 in a log: its train-loss lines and its validation block (the log's first 'Epoch: 1/n' block)."""
    lines = _log(path)
    end = next(i for i, line in enumerate(lines) if line.startswith(f"Epoch: 1/{n_epochs} "))
    start = max(i for i in range(end) if lines[i].startswith("Epoch: "))
    train = [line for line in lines[start:end] if line.startswith("train ")]
    val = [lines[end]] + list(itertools.takewhile(lambda line: line.startswith("val "), lines[end + 1:]))
    assert train and len(val) >= 3
    return train, val


@pytest.mark.parametrize("mod", ["amid_amd.train_sr", "amid_amd.train_sr_dr"])
def test_cli_resume_equals_uninterrupted(tmp_path, mod):
    base = _data(tmp_path, mod.endswith("_dr")) + ["--seeds", "2"]
    A, Bd, la, lb = tmp_path / "A", tmp_path / "B", tmp_path / "logA", tmp_path / "logB"
    _cli(mod, base + ["--epoch", "2", "--save_dir", str(A), "-md", str(la)])
    _cli(mod, base + ["--epoch", "1", "--save_dir", str(Bd), "--save_every", "1", "-md", str(lb)])
    _cli(mod, base + ["--epoch", "2", "--resume", str(Bd / "seed0" / "last.pt"), "--save_dir", str(Bd), "-md", str(lb)])
    assert _seed0_epoch1(la / "log0.txt", 2) == _seed0_epoch1(lb / "log0.txt", 2)
    sa, sb = _log(la / "log_all.txt"), _log(lb / "log_all.txt")          # (B's holds the first run's summary too)
    assert len(sa) > 0 and sb[-len(sa):] == sa
    for s in ("seed0", "seed1"):
        for f in ("last.pt", "best_d1.pt", "best_d2.pt"):
            _assert_same(torch.load(A / s / f, weights_only=True), torch.load(Bd / s / f, weights_only=True))
    shutil.rmtree(A)
    shutil.rmtree(Bd)


def test_best_file_is_the_best_epoch(tmp_path):
    from amid_amd.model_seq import SASRec
    base = _data(tmp_path, False) + ["--seeds", "1", "-md", str(tmp_path / "log")]
    C, snaps = tmp_path / "C", []
    for e in range(3):                    # one epoch per process: every epoch's last.pt is kept
        _cli("amid_amd.train_sr", base + ["--epoch", str(e + 1), "--save_dir", str(C), "--save_every", "1"]
             + (["--resume", str(snaps[-1])] if snaps else []))
        snaps.append(tmp_path / f"ep{e}.pt")
        os.replace(C / "seed0" / "last.pt", snaps[-1])
    states = [torch.load(p, weights_only=True) for p in snaps]
    mrr = [s["extra"]["metrics"]["d1"][6] for s in states]
    e_best = max(e for e in range(3) if all(mrr[e] >= mrr[j] for j in range(e)))
    best = torch.load(C / "seed0" / "best_d1.pt", weights_only=True)
    params = states[e_best]["engine"]["parameters"]
    assert list(best) == list(params)
    for k in params:
        assert torch.equal(best[k], params[k]), k
    # the weights-only file in a fresh model recommends what that epoch's model recommends
    mk = lambda seed: SASRec(2 * 895510, 64, 2 * 447410, 64, 20, 16, 32, False, False, 0.5, 0.5, seed=seed).eval()     # noqa: E731
    m1, m2 = mk(1), mk(2)
    m1.load_state_dict(best, strict=True)
    m2.load_training_state(states[e_best])
    g = torch.Generator().manual_seed(0)
    s1, s2 = torch.randint(1, 400, (8, 20), generator=g).cuda(), torch.randint(400, 900, (8, 20), generator=g).cuda()
    dom = torch.randint(0, 2, (8,), generator=g).cuda()
    i1, c1 = m1.recommend(s1, s2, dom, k=10)
    i2, c2 = m2.recommend(s1, s2, dom, k=10)
    assert torch.equal(i1, i2) and torch.equal(c1, c2)
    shutil.rmtree(C)
    for p in snaps:
        p.unlink()
