"""Full-catalog evaluation and top-K recommendation (csrc/full_rank.hip, SasrecEngine.enqueue_full_rank / enqueue_topk,
SASRec.full_ranks / recommend, train_sr.py --full_rank): exact integer recounts from the kernel's own scores, the sampled path's ranks as a
lower bound (equal where the sample is the whole candidate set), the fp64 oracle, the whole table, and the command line."""
import json

import numpy as np
import pytest
import torch

from oracle import amid_oracle as orc

pytestmark = pytest.mark.gpu
FIX = 1e-7


def _lib():
    from amid_amd._lib import lib
    return lib()


class Scorer:
    """Random predictModule weights + a table, and direct calls of the two entry points on torch's current stream."""

    def __init__(self, n_rows, D, hid, seed, dup_rows=0):
        g = torch.Generator().manual_seed(seed)
        self.D, self.hid, self.n_rows = D, hid, n_rows
        self.table = torch.randn(n_rows, D, generator=g)
        if dup_rows:                                 # rows 2 i + 1 copy rows 2 i: equal scores, ties broken by the id
            self.table[1:2 * dup_rows:2] = self.table[0:2 * dup_rows:2]
        a1, a2 = 1.0 / (2 * D) ** 0.5, 1.0 / hid ** 0.5
        self.w1 = (torch.rand(hid, 2 * D, generator=g) * 2 - 1) * a1
        self.b1 = (torch.rand(hid, generator=g) * 2 - 1) * a1
        self.w2 = (torch.rand(1, hid, generator=g) * 2 - 1) * a2
        self.b2 = (torch.rand(1, generator=g) * 2 - 1) * a2
        self.cu = {k: getattr(self, k).cuda() for k in ("table", "w1", "b1", "w2", "b2")}

    def _ws(self, B, n1, n2, k):
        nb = _lib().value("amid_full_rank_workspace_bytes", B, n1, n2, self.hid, k)
        return torch.empty(nb, dtype=torch.uint8, device="cuda")

    def _w(self):
        c = self.cu
        return (c["table"].data_ptr(), self.n_rows, c["w1"].data_ptr(), c["b1"].data_ptr(), c["w2"].data_ptr(), c["b2"].data_ptr(), self.D,
                self.hid)

    def rank(self, u, pos, dom, pools, own=None, own_off=None, rows=None, want_scores=True):
        B = u.shape[0]
        p1, p2 = pools
        rank = torch.empty(B, dtype=torch.int32, device="cuda")
        raw = torch.empty_like(rank)
        ncol = max(p1.numel(), p2.numel())
        sc = torch.full((B, ncol), float("nan"), device="cuda") if want_scores else None
        flags = torch.zeros(1, dtype=torch.int32, device="cuda")
        ws = self._ws(B, p1.numel(), p2.numel(), 0)
        ptr = lambda t: None if t is None else t.data_ptr()       # noqa: E731
        _lib().call("amid_full_rank_f32", u.data_ptr(), 0, pos.data_ptr(), dom.data_ptr(), B, p1.data_ptr(), p1.numel(), p2.data_ptr(),
                    p2.numel(), ptr(own), ptr(own_off), ptr(rows), *self._w(), FIX, ws.data_ptr(), flags.data_ptr(), rank.data_ptr(),
                    raw.data_ptr(), ptr(sc), ncol if want_scores else 0, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert int(flags.item()) == 0
        return rank.cpu(), raw.cpu(), (sc.cpu() if want_scores else None)

    def topk(self, u, dom, pools, k, own=None, own_off=None, rows=None, exclude=True):
        B = u.shape[0]
        p1, p2 = pools
        ids = torch.empty(B, k, dtype=torch.int64, device="cuda")
        sc = torch.empty(B, k, device="cuda")
        flags = torch.zeros(1, dtype=torch.int32, device="cuda")
        ws = self._ws(B, p1.numel(), p2.numel(), k)
        ptr = lambda t: None if t is None else t.data_ptr()       # noqa: E731
        _lib().call("amid_topk_f32", u.data_ptr(), 0, dom.data_ptr(), B, p1.data_ptr(), p1.numel(), p2.data_ptr(), p2.numel(), ptr(own),
                    ptr(own_off), ptr(rows), *self._w(), k, 1 if exclude else 0, ws.data_ptr(), flags.data_ptr(), ids.data_ptr(), sc.data_ptr(),
                    torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert int(flags.item()) == 0
        return ids.cpu(), sc.cpu()


def _own_csr(own_lists):
    off = np.zeros(len(own_lists) + 1, dtype=np.int32)
    np.cumsum([len(o) for o in own_lists], out=off[1:])
    flat = np.concatenate([np.asarray(o, dtype=np.int64) for o in own_lists]) if off[-1] else np.zeros(1, np.int64)
    return torch.from_numpy(flat).cuda(), torch.from_numpy(off).cuda()


def _cpu_topk(scores_row, ids_row, k):
    """A stable sort of (score desc, id asc); padded with (-1, -inf)."""
    order = sorted(range(len(ids_row)), key=lambda i: (-float(scores_row[i]), int(ids_row[i])))[:k]
    ids = [int(ids_row[i]) for i in order] + [-1] * (k - len(order))
    sc = [float(scores_row[i]) for i in order] + [float("-inf")] * (k - len(order))
    return ids, sc


@pytest.mark.parametrize("N,B,D,hid", [(1, 1, 128, 32), (17, 7, 64, 16), (1000, 256, 128, 32), (1000, 7, 64, 64), (1300, 7, 128, 64)])
def test_exact_recount_and_topk_from_the_kernels_own_scores(N, B, D, hid):
    n_rows = N + 50
    sc = Scorer(n_rows, D, hid, seed=N + B + D, dup_rows=min(N // 2, 20))
    rng = np.random.default_rng(N + B)
    pool1 = torch.arange(N, dtype=torch.int64)                             # domain 0: rows 0 .. N - 1 (the duplicated pairs among them)
    pool2 = torch.from_numpy(np.sort(rng.choice(n_rows, size=max(1, N // 2), replace=False))).long()
    dom = torch.from_numpy(rng.integers(0, 2, B)).long()
    pools = [pool1, pool2]
    pos, own_lists = [], []
    for b in range(B):
        p = pools[int(dom[b])]
        pos.append(int(p[rng.integers(0, len(p))]))
        extra = rng.choice(n_rows, size=min(5, n_rows), replace=False)
        own_lists.append(np.unique(np.concatenate([[pos[-1]], extra])))
    pos = torch.tensor(pos)
    u = torch.randn(B, D, generator=torch.Generator().manual_seed(7)) * 0.5
    own, off = _own_csr(own_lists)
    rows = torch.arange(B, dtype=torch.int32).cuda()
    pc = (pool1.cuda(), pool2.cuda())
    rank, raw, scores = sc.rank(u.cuda(), pos.cuda(), dom.cuda(), pc, own, off, rows)
    for b in range(B):
        p = pools[int(dom[b])]
        s = scores[b, :len(p)]
        assert not torch.isnan(s).any()
        pos_i = int((p == pos[b]).nonzero()[0, 0])
        p0 = s[pos_i]
        keep = torch.tensor([int(c) not in set(own_lists[b].tolist()) for c in p])
        thr = torch.tensor(float(p0), dtype=torch.float32) - torch.tensor(FIX, dtype=torch.float32)
        assert int(rank[b]) == int(((s > thr) & keep).sum()), b
        assert int(raw[b]) == int(((s > p0) & keep).sum()), b
    for k in sorted({1, 10, 256, N + 3} & set(range(1, 257))):
        for excl in (True, False):
            ids, ts = sc.topk(u.cuda(), dom.cuda(), pc, k, own, off, rows, exclude=excl)
            for b in range(B):
                p = pools[int(dom[b])]
                s = scores[b, :len(p)]
                sel = [i for i in range(len(p)) if not (excl and int(p[i]) in set(own_lists[b].tolist()))]
                want_ids, want_s = _cpu_topk(s[sel], p[sel], k)
                assert ids[b].tolist() == want_ids, (k, excl, b)
                assert ts[b].tolist() == want_s, (k, excl, b)


def test_topk_ties_go_to_the_lower_id():
    sc = Scorer(64, 64, 16, seed=3, dup_rows=32)                          # every row 2 i + 1 equals row 2 i
    u = torch.randn(5, 64, generator=torch.Generator().manual_seed(1))
    pool = torch.arange(64, dtype=torch.int64).cuda()
    ids, s = sc.topk(u.cuda(), torch.zeros(5, dtype=torch.int64).cuda(), (pool, pool), 64, exclude=False)
    for b in range(5):
        assert ids[b].tolist()[0] % 2 == 0
        for i in range(0, 64, 2):                                          # equal scores come in (even, odd) pairs, even first
            assert s[b, i] == s[b, i + 1] and ids[b, i] + 1 == ids[b, i + 1]


def test_whole_table_is_deterministic_and_splits_merge():
    n_rows, D, hid, B = 894820, 128, 32, 256
    sc = Scorer(n_rows, D, hid, seed=11)
    g = torch.Generator().manual_seed(5)
    u = (torch.randn(B, D, generator=g) * 0.5).cuda()
    dom = torch.randint(0, 2, (B,), generator=g).cuda()
    pos = torch.randint(0, n_rows, (B,), generator=g).cuda()
    full = torch.arange(n_rows, dtype=torch.int64).cuda()
    h1, h2 = full[: n_rows // 2].contiguous(), full[n_rows // 2:].contiguous()
    r1, w1, _ = sc.rank(u, pos, dom, (full, full), want_scores=False)
    r2, w2, _ = sc.rank(u, pos, dom, (full, full), want_scores=False)
    assert torch.equal(r1, r2) and torch.equal(w1, w2)
    # the same count over the two halves, summed on the host (the positive's score does not depend on the pool)
    ra, wa, _ = sc.rank(u, pos, dom, (h1, h1), want_scores=False)
    rb, wb, _ = sc.rank(u, pos, dom, (h2, h2), want_scores=False)
    assert torch.equal(r1, ra + rb) and torch.equal(w1, wa + wb)
    k = 10
    i1, s1 = sc.topk(u, dom, (full, full), k, exclude=False)
    i2, s2 = sc.topk(u, dom, (full, full), k, exclude=False)
    assert torch.equal(i1, i2) and torch.equal(s1, s2)
    ia, sa = sc.topk(u, dom, (h1, h1), k, exclude=False)
    ib, sb = sc.topk(u, dom, (h2, h2), k, exclude=False)
    for b in range(B):
        want_ids, want_s = _cpu_topk(torch.cat((sa[b], sb[b])), torch.cat((ia[b], ib[b])), k)
        assert i1[b].tolist() == want_ids and s1[b].tolist() == want_s


def test_scores_against_the_fp64_oracle():
    """Plain SASRec: the full-catalog scores of the oracle's eval-mode user vectors within 2e-6 of oracle.predict_module."""
    from amid_amd.engine import SasrecEngine
    n_items, D, T, hid, B = 3000, 128, 20, 32, 16
    P = orc.random_params(orc.sasrec_param_shapes(n_items, D, T, hid), seed=21)
    eng = SasrecEngine(n_items, D, T, hid, device="cuda:0", lr=1e-3, seed=5)
    eng.load_state_dict(P)
    b = orc.synthetic_batch(B, T, n_items - 1, pad_id=n_items - 1, neg=4, seed=9)
    taps = {}
    with torch.no_grad():
        orc.sasrec_forward(P, b["i_node"], b["neg_samples"], b["seq_d1"], b["seq_d2"], None, taps)
    dom = b["domain_id"]
    u = torch.where(dom[:, None] != 0, taps["u2"], taps["u1"]).float().contiguous()
    pool = torch.arange(0, n_items, 3, dtype=torch.int64)
    sc = Scorer.__new__(Scorer)
    sc.D, sc.hid, sc.n_rows = D, hid, n_items
    sc.cu = {"table": eng.table, "w1": eng.dense.view("predictModule.fc.0.weight"), "b1": eng.dense.view("predictModule.fc.0.bias"),
             "w2": eng.dense.view("predictModule.fc.2.weight"), "b2": eng.dense.view("predictModule.fc.2.bias")}
    _, _, s = sc.rank(u.cuda(), b["i_node"].cuda(), dom.cuda(), (pool.cuda(), pool.cuda()))
    Pd = {k: v.double() for k, v in P.items() if k.startswith("predictModule")}
    items = P["item_emb_layer.emb_item.weight"].double()[pool].unsqueeze(0).expand(B, -1, -1)
    with torch.no_grad():
        want, _ = orc.predict_module(u.double(), u.double(), items, Pd)
    assert float((s[:, :pool.numel()].double() - want).abs().max()) < 2e-6


def _write_csv(path, n, rng, lo1, hi1, lo2, hi2):
    rows = ["user_id,seq_d1,seq_d2,domain_id"]
    for u in range(n):
        dom = int(rng.random() < 0.5)
        l1 = int(rng.integers(1 if dom == 0 else 0, 9))
        l2 = int(rng.integers(1 if dom == 1 else 0, 9))
        s1 = [int(x) for x in rng.integers(lo1, hi1, l1)]
        s2 = [int(x) for x in rng.integers(lo2, hi2, l2)]
        rows.append(f'{u},"{json.dumps(s1)}","{json.dumps(s2)}",{dom}')
    with open(path, "w") as f:
        f.write("\n".join(rows) + "\n")


def _sampled_ranks(model, vb, ep):
    """test()'s sampled ranks of the same epoch (same negatives), through eval_ranks or model.forward."""
    from amid_amd.utils import device_positive_ranks
    fused = model.eval_ranks(ep, FIX)
    if fused is not None:
        return fused["rank"].reshape(-1)
    out = []
    for i in range(ep["seq_d1"].shape[0]):
        outs = model(ep["user_node"][i], ep["i_node"][i], ep["neg_samples"][i], ep["seq_d1"][i], ep["seq_d2"][i], None, None, False)
        B = ep["i_node"].shape[1]
        out.append(device_positive_ranks(outs[0].reshape(B, -1), outs[1].reshape(B, -1), ep["domain_id"][i], FIX))
    return torch.cat(out)


@pytest.mark.parametrize("kind", ["sasrec", "itc", "dr", "bert4rec"])
def test_full_ranks_against_the_sampled_path(tmp_path, kind):
    from amid_amd import model_seq
    from amid_amd.dataset_seq import DeviceBatches, DualDomainSeqDataset
    rng = np.random.default_rng(4)
    # pools of 38 items per domain and 30 negatives: a row whose own sequence holds 8 distinct items has exactly 30 candidates, all sampled
    rows = ["user_id,seq_d1,seq_d2,domain_id"]
    for u in range(128):
        dom = int(rng.random() < 0.5)
        ranges = ((1, 39), (39, 77))
        own_len = 8 if u % 2 == 0 else int(rng.integers(1, 8))
        seqs = [[int(x) for x in rng.choice(np.arange(*ranges[d]), size=own_len if d == dom else int(rng.integers(0, 9)), replace=False)]
                for d in (0, 1)]
        rows.append(f'{u},"{json.dumps(seqs[0])}","{json.dumps(seqs[1])}",{dom}')
    (tmp_path / "toy_test.csv").write_text("\n".join(rows) + "\n")
    ds = DualDomainSeqDataset(seq_len=20, isTrain=False, neg_nums=30, long_length=7, pad_id=101, seed=3, csv_path=str(tmp_path / "toy_test.csv"))
    bs = 32
    D = 128 if kind == "bert4rec" else 64
    kw = dict(isItC=kind == "itc")
    cls = model_seq.BERT4Rec if kind == "bert4rec" else model_seq.SASRec
    extra = {"isDR": True} if kind == "dr" else {}
    model = cls(10, D, 120, D, 20, 16, bs, False, kw["isItC"], 0.5, 0.3, seed=2, **extra)
    model.eval()
    vb = DeviceBatches(ds, bs, shuffle=False, device="cuda:0", seed=9)
    ep = vb.epoch_tensors()
    with torch.no_grad():
        sampled = _sampled_ranks(model, vb, ep).cpu()
    full = model.full_ranks(ep, vb, FIX)
    fr = full["rank"].reshape(-1).cpu()
    assert fr.shape == sampled.shape
    assert bool((fr >= sampled).all())
    neg = ep["neg_samples"].reshape(-1, 30).cpu()
    dom = ep["domain_id"].reshape(-1).cpu()
    n_eq = 0
    for r in range(fr.numel()):
        cand = set(ds.pool[int(dom[r])].tolist()) - set(ds.own_items[r].tolist())
        if set(neg[r].tolist()) == cand:
            assert int(fr[r]) == int(sampled[r]), r
            n_eq += 1
    assert n_eq >= 5, n_eq


def test_recommend_excludes_history_and_matches_the_full_scores():
    from amid_amd import model_seq
    n = 200
    model = model_seq.SASRec(10, 64, n, 64, 20, 16, 8, False, False, 0.5, 0.5, seed=4)
    model.eval()
    g = torch.Generator().manual_seed(2)
    B = 8
    s1 = torch.randint(1, n - 1, (B, 20), generator=g)
    s2 = torch.randint(1, n - 1, (B, 20), generator=g)
    dom = torch.randint(0, 2, (B,), generator=g)
    ids, sc = model.recommend(s1.cuda(), s2.cuda(), dom.cuda(), k=n)
    ids_all, sc_all = model.recommend(s1.cuda(), s2.cuda(), dom.cuda(), k=n, exclude_history=False)
    assert bool((ids_all >= 0).all())
    for b in range(B):
        hist = set((s2[b] if dom[b] else s1[b]).tolist())
        got = [i for i in ids[b].tolist() if i >= 0]
        assert len(got) == n - len(hist) and not (set(got) & hist)
        assert ids[b, len(got):].eq(-1).all() and torch.isinf(sc[b, len(got):]).all()
        assert sorted(ids_all[b].tolist()) == list(range(n))
        # the excluded ranking is the unexcluded one with the history removed, with the same scores
        assert [i for i in ids_all[b].tolist() if i not in hist] == got
        keep = torch.tensor([i not in hist for i in ids_all[b].tolist()])
        assert torch.equal(sc_all[b][keep], sc[b, :len(got)])
    with pytest.raises(ValueError):
        model.recommend(s1.cuda(), s2.cuda(), dom.cuda(), k=0)


@pytest.mark.parametrize("model,emb,extra,dr", [("sasrec", "64", [], False), ("bert4rec", "128", [], False),
                                                ("sasrec", "64", ["--isItC", "True", "--ts2", "0.4"], False), ("sasrec", "64", [], True)])
def test_cli_full_rank(tmp_path, model, emb, extra, dr):
    rng = np.random.default_rng(0)
    root = tmp_path / "amazon_dataset"
    root.mkdir()
    if dr:
        from amid_amd.train_sr_dr import main
        from tests.test_gpu_module import _write_csv as write_dr
        write_dr(root / "toy_train75.csv", 150, rng, 1, 300, 300, 700)
        write_dr(root / "toy_train75_DR.csv", 120, rng, 1, 300, 300, 700, ob_label=True)
        write_dr(root / "toy_test.csv", 64, rng, 1, 300, 300, 700)
        extra = ["--isDR", "True"]
    else:
        from amid_amd.train_sr import main
        _write_csv(root / "toy_train75.csv", 300, rng, 1, 400, 400, 900)
        _write_csv(root / "toy_test.csv", 80, rng, 1, 400, 400, 900)
    summary = main(["--data_root", str(tmp_path), "-ds", "amazon", "-dm", "toy", "--overlap_ratio", "0.75", "--model", model,
                    "--bs", "32", "--seq_len", "20", "--emb_dim", emb, "--hid_dim", "16", "--epoch", "1", "--neg_nums", "19",
                    "--seeds", "1", "-md", str(tmp_path / "model"), "--full_rank"] + extra)
    best = summary[0]
    for d in ("d1", "d2"):
        for n in ("HR@1", "HR@5", "HR@10", "MRR"):
            assert (f"{d}_full", n) in best
            v = best[(f"{d}_full", n)]
            assert 0.0 <= v <= 1.0
        for n in ("HR@1", "HR@5", "HR@10"):
            assert best[(f"{d}_full", n)] <= best[(d, n)] + 1e-12
    assert all(0.0 <= v <= 1.0 for v in best.values())


def test_cli_full_rank_refuses_joint_jobs(tmp_path):
    from amid_amd.train_sr import main
    with pytest.raises(SystemExit, match="full_rank"):
        main(["--data_root", str(tmp_path), "-dm", "a+b", "--full_rank", "--seeds", "1"])
