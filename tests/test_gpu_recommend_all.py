"""Top-K for a whole dataset (csrc/own_sets.hip, csrc/full_rank.hip amid_topk_items_f32 / amid_topk_users_f32, SasrecEngine.topk_epoch,
SASRec.recommend_all, recommend.py): the own sets against numpy, items-then-users against amid_topk_f32, recommend_all against a loop of
recommend() (graph and eager, before and after a train step), the launch record, the full ranks, and the command line."""
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


# ---- 1. own sets ---------------------------------------------------------------------------------------------------------------------------
def _own_case(B, T, seed):
    """Rows cycling through: all pad, all one id, all distinct, random with repeats (a few ids beyond 2^31 among them); mixed domains."""
    rng = np.random.default_rng(seed)
    pad = 10 ** 6 + 1
    seqs = np.empty((2, B, T), dtype=np.int64)
    for d in range(2):
        for b in range(B):
            kind = (b + d) % 4
            if kind == 0:
                row = np.full(T, pad)
            elif kind == 1:
                row = np.full(T, int(rng.integers(1, 50)))
            elif kind == 2:
                row = rng.permutation(np.arange(1, 4 * T + 1))[:T] + 1000 * d
            else:
                row = rng.integers(1, max(2, T // 2 + 1), T)
                row[rng.random(T) < 0.3] = pad
                if T > 2:
                    row[int(rng.integers(0, T))] = (1 << 40) + int(rng.integers(0, 3))
            seqs[d, b] = row
    dom = rng.integers(0, 2, B).astype(np.int64)
    if B > 1:
        dom[0], dom[1] = 0, 1
    return seqs, dom


@pytest.mark.parametrize("B,T", [(1, 1), (3, 5), (7, 64), (5, 200), (64, 20), (2, 512)])
def test_own_sets_against_numpy(B, T):
    seqs, dom = _own_case(B, T, seed=B * 1000 + T)
    s1, s2, dm = (torch.from_numpy(a).cuda() for a in (seqs[0], seqs[1], dom))
    own = torch.full((B * T,), -7, dtype=torch.int64, device="cuda")
    off = torch.full((B + 1,), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    _lib().call("amid_own_from_seq_i64", s1.data_ptr(), s2.data_ptr(), dm.data_ptr(), B, T, cnt.data_ptr(), own.data_ptr(), off.data_ptr(),
                torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    want = [np.unique(seqs[int(dom[b] != 0), b]) for b in range(B)]
    want_off = np.zeros(B + 1, dtype=np.int64)
    np.cumsum([len(w) for w in want], out=want_off[1:])
    assert off.cpu().numpy().tolist() == want_off.tolist()
    n = int(want_off[-1])
    assert own[:n].cpu().numpy().tolist() == np.concatenate(want).tolist()
    # exactly the set recommend() builds on the host side of the ABI
    srt = torch.sort(torch.where(dm.unsqueeze(1) != 0, s2, s1), dim=1).values
    keep = torch.ones_like(srt, dtype=torch.bool)
    keep[:, 1:] = srt[:, 1:] != srt[:, :-1]
    assert torch.equal(own[:n], srt[keep])


# ---- 2. items then users = amid_topk_f32 ---------------------------------------------------------------------------------------------------
class Scorer:
    def __init__(self, n_rows, D, hid, seed):
        g = torch.Generator().manual_seed(seed)
        self.D, self.hid, self.n_rows = D, hid, n_rows
        a1, a2 = 1.0 / (2 * D) ** 0.5, 1.0 / hid ** 0.5
        self.table = torch.randn(n_rows, D, generator=g).cuda()
        self.table[1:21:2] = self.table[0:20:2]              # a few equal rows: equal scores, ties broken by the id
        self.w1 = ((torch.rand(hid, 2 * D, generator=g) * 2 - 1) * a1).cuda()
        self.b1 = ((torch.rand(hid, generator=g) * 2 - 1) * a1).cuda()
        self.w2 = ((torch.rand(1, hid, generator=g) * 2 - 1) * a2).cuda()
        self.b2 = ((torch.rand(1, generator=g) * 2 - 1) * a2).cuda()
        self.flags = torch.zeros(1, dtype=torch.int32, device="cuda")

    def ws(self, B, n1, n2, k):
        return torch.empty(_lib().value("amid_full_rank_workspace_bytes", B, n1, n2, self.hid, k), dtype=torch.uint8, device="cuda")

    def _tail(self, k, excl, ws, ids, sc):
        return (self.table.data_ptr(), self.n_rows, self.w1.data_ptr(), self.b1.data_ptr(), self.w2.data_ptr(), self.b2.data_ptr(), self.D,
                self.hid, k, 1 if excl else 0, ws.data_ptr(), self.flags.data_ptr(), ids.data_ptr(), sc.data_ptr(),
                torch.cuda.current_stream().cuda_stream)

    def run(self, entry, u, dom, pools, own, off, rows, k, excl, ws):
        B = u.shape[0]
        p1, p2 = pools
        ids = torch.full((B, k), -9, dtype=torch.int64, device="cuda")
        sc = torch.full((B, k), float("nan"), device="cuda")
        _lib().call(entry, u.data_ptr(), 0, dom.data_ptr(), B, p1.data_ptr(), p1.numel(), p2.data_ptr(), p2.numel(), own.data_ptr(),
                    off.data_ptr(), rows.data_ptr(), *self._tail(k, excl, ws, ids, sc))
        torch.cuda.synchronize()
        assert int(self.flags.item()) == 0
        return ids, sc

    def items(self, B, pools, ws):
        p1, p2 = pools
        _lib().call("amid_topk_items_f32", B, p1.data_ptr(), p1.numel(), p2.data_ptr(), p2.numel(), self.table.data_ptr(), self.n_rows,
                    self.w1.data_ptr(), self.D, self.hid, ws.data_ptr(), self.flags.data_ptr(), torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("N,B,D,hid", [(1, 1, 128, 32), (17, 7, 64, 16), (1300, 33, 128, 64)])
def test_items_then_users_equals_topk(N, B, D, hid):
    n_rows = N + 50
    sc = Scorer(n_rows, D, hid, seed=N + B)
    rng = np.random.default_rng(N)
    p1 = torch.arange(N, dtype=torch.int64).cuda()
    p2 = torch.from_numpy(np.sort(rng.choice(n_rows, size=max(1, N // 2), replace=False))).long().cuda()      # N 17: 8 candidates < k 10
    dom = torch.from_numpy(rng.integers(0, 2, B)).long().cuda()
    own_lists = [np.unique(rng.choice(n_rows, size=min(6, n_rows), replace=False)) for _ in range(B)]
    off = np.zeros(B + 1, dtype=np.int32)
    np.cumsum([len(o) for o in own_lists], out=off[1:])
    own, off = torch.from_numpy(np.concatenate(own_lists)).cuda(), torch.from_numpy(off).cuda()
    rows = torch.arange(B, dtype=torch.int32).cuda()
    g = torch.Generator().manual_seed(7)
    u, u2 = (torch.randn(B, D, generator=g) * 0.5).cuda(), (torch.randn(B, D, generator=g) * 0.5).cuda()
    padded = False
    for k in (1, 10, 256):
        for excl in (True, False):
            want = sc.run("amid_topk_f32", u, dom, (p1, p2), own, off, rows, k, excl, sc.ws(B, N, p2.numel(), k))
            want2 = sc.run("amid_topk_f32", u2, dom, (p1, p2), own, off, rows, k, excl, sc.ws(B, N, p2.numel(), k))
            ws = sc.ws(B, N, p2.numel(), k)
            ws.fill_(0xff)                                   # nothing of the split's workspace comes from an earlier whole call
            sc.items(B, (p1, p2), ws)
            got = sc.run("amid_topk_users_f32", u, dom, (p1, p2), own, off, rows, k, excl, ws)
            got2 = sc.run("amid_topk_users_f32", u2, dom, (p1, p2), own, off, rows, k, excl, ws)       # a second batch on the same item halves
            for (wi, wsc), (gi, gsc) in ((want, got), (want2, got2)):
                assert torch.equal(wi, gi) and torch.equal(wsc, gsc), (k, excl)
            padded = padded or bool((want[0] == -1).any())
            assert not bool((want[0] == -9).any()) and not bool(torch.isnan(want[1]).any())
    assert padded == (N < 256)                               # a pool with fewer than k candidates: the -1 / -inf padding is compared


# ---- 3. recommend_all = a loop of recommend() ----------------------------------------------------------------------------------------------
def _model(kind, T, bs):
    from amid_amd import model_seq
    base = kind.rstrip("0123456789")
    D = 128 if (base == "bert4rec" or kind.endswith("128")) else 64
    cls = model_seq.BERT4Rec if base == "bert4rec" else model_seq.SASRec
    extra = {"isDR": True} if base == "dr" else {}
    model = cls(10, D, 120, D, T, 16, bs, base == "inc", base == "itc", 0.5, 0.3, seed=2, **extra)
    model.eval()
    return model


def _users(n, B, T, seed):
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name in ("seq_d1", "seq_d2"):
        s = torch.randint(1, 101, (n, B, T), generator=g)
        lens = torch.randint(0, min(T, 12) + 1, (n, B, 1), generator=g)
        s[torch.arange(T).view(1, 1, T) < T - lens] = 101   # left-padded with the pad id
        out[name] = s.cuda()
    out["domain_id"] = torch.randint(0, 2, (n, B), generator=g).cuda()
    return out


def _loop(model, users, **kw):
    n = users["seq_d1"].shape[0]
    outs = [model.recommend(users["seq_d1"][i], users["seq_d2"][i], users["domain_id"][i], **kw) for i in range(n)]
    return torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs])


@pytest.mark.parametrize("kind,T", [("sasrec", 20), ("itc", 20), ("dr", 20), ("inc", 20), ("bert4rec", 20), ("sasrec128", 70), ("sasrec", 70),
                                    ("bert4rec", 70)])
def test_recommend_all_equals_a_loop_of_recommend(kind, T):
    """(8, 20): the fused evaluation's user vectors; sasrec128 at 70 tokens: its seven-launch long form; sasrec (D 64) and bert4rec at 70:
    enqueue_prepare + enqueue_forward, captured as well."""
    n, B, k = 3, 8, 10
    model = _model(kind, T, B)
    users = _users(n, B, T, seed=T + len(kind))
    pools = (torch.arange(1, 61, dtype=torch.int64).cuda(), torch.arange(40, 102, dtype=torch.int64).cuda())
    variants = [dict(k=k, pool=pools, exclude_history=True)]
    if kind == "sasrec":
        variants += [dict(k=5, pool=None, exclude_history=False), dict(k=256, pool=pools[0], exclude_history=True)]
    for rnd in range(2):
        for kw in variants:
            want_i, want_s = _loop(model, users, **kw)
            got_i, got_s = model.recommend_all(users, use_graph=True, **kw)
            eag_i, eag_s = model.recommend_all(users, use_graph=False, **kw)
            assert got_i.shape == (n, B, kw["k"]) and got_i.dtype == torch.int64 and got_s.dtype == torch.float32
            assert torch.equal(got_i, want_i) and torch.equal(got_s, want_s), (rnd, kw["k"])
            assert torch.equal(eag_i, want_i) and torch.equal(eag_s, want_s), (rnd, kw["k"])
            assert bool((got_i[..., 0] >= 0).all())
        if rnd == 0:
            # one train step: the second round sees other weights (the item halves are rebuilt, the captured graphs replayed again)
            before = want_s.clone()
            model.train()
            label = torch.zeros(B, 2, device="cuda")
            label[:, 0] = 1.0
            g = torch.Generator().manual_seed(1)
            pos = torch.randint(1, 101, (B,), generator=g).cuda()
            neg = torch.randint(1, 101, (B, 1), generator=g).cuda()
            model.train_step(pos, neg, users["seq_d1"][0][:, -20:].contiguous(), users["seq_d2"][0][:, -20:].contiguous(), label,
                             users["domain_id"][0])
            model.eval()
    assert not torch.equal(before, want_s)                   # the step did change what is recommended


def test_recommend_all_checks_its_arguments():
    model = _model("itc", 20, 8)
    users = _users(2, 8, 20, seed=1)
    with pytest.raises(ValueError, match="k must be in 1..256"):
        model.recommend_all(users, k=0)
    with pytest.raises(ValueError, match="k must be in 1..256"):
        model.recommend_all(users, k=257)
    with pytest.raises(ValueError, match="exactly bs = 8"):
        model.recommend_all({k: v[:, :5] for k, v in users.items()})


# ---- 4. launch record ----------------------------------------------------------------------------------------------------------------------
def test_launch_record_of_an_eager_recommend_all(monkeypatch):
    L = _lib()
    model = _model("sasrec", 20, 8)
    users = _users(3, 8, 20, seed=3)
    names = []
    orig = L.call

    def call(name, *args):
        names.append(name)
        return orig(name, *args)

    monkeypatch.setattr(L, "call", call)
    try:
        model.recommend_all(users, k=10, use_graph=False)
    finally:
        monkeypatch.undo()
    assert names.count("amid_topk_items_f32") == 1
    assert names.count("amid_topk_users_f32") == 3
    assert names.count("amid_own_from_seq_i64") == 3
    assert "amid_topk_f32" not in names


# ---- 5. consistency with full_ranks --------------------------------------------------------------------------------------------------------
def test_positive_in_top_k_exactly_when_its_full_rank_is_below_k(tmp_path):
    """The positive is among the k best of (pool - history) exactly when fewer than k candidates of (pool - own items) score above it --
    two independent launch sequences (top-K lists against counts).  Rows where another candidate's fp32 score equals the positive's bit
    for bit are left out (the top-K breaks that tie by the id, the rank counts strictly above); at most 5 % of the rows may be."""
    from amid_amd import model_seq
    from amid_amd.dataset_seq import DeviceBatches, DualDomainSeqDataset
    rng = np.random.default_rng(5)
    rows = ["user_id,seq_d1,seq_d2,domain_id"]
    for u in range(64):
        dom = int(rng.random() < 0.5)
        seqs = [[int(x) for x in rng.integers(lo, hi, int(rng.integers(1 if d == dom else 0, 9)))] for d, (lo, hi) in enumerate(((1, 151), (151, 301)))]
        rows.append(f'{u},"{json.dumps(seqs[0])}","{json.dumps(seqs[1])}",{dom}')
    (tmp_path / "toy_test.csv").write_text("\n".join(rows) + "\n")
    T, D, hid, n_rows, k = 20, 64, 16, 310, 10                  # seq_len 20 > the longest row (8): no history is cut off
    ds = DualDomainSeqDataset(seq_len=T, isTrain=False, neg_nums=5, long_length=7, pad_id=301, seed=3, csv_path=str(tmp_path / "toy_test.csv"))
    model = model_seq.SASRec(10, D, n_rows, D, T, hid, 64, False, False, 0.5, 0.5, seed=2)
    model.load_state_dict({n: v.cuda() for n, v in orc.random_params(orc.sasrec_param_shapes(n_rows, D, T, hid), seed=3).items()})
    model.eval()
    vb = DeviceBatches(ds, 64, shuffle=False, device="cuda:0", seed=5)
    ep = vb.epoch_tensors()
    assert ep["seq_d1"].shape[0] == 1
    pools = (vb.pool[0], vb.pool[1])
    raw = model.full_ranks(ep, vb, FIX)["rank_raw"].reshape(-1).cpu()
    ids, _ = model.recommend_all(ep, k=k, pool=pools)
    ids = ids.reshape(64, k).cpu()
    # the kernel's own scores of every candidate, the history included: rows where the positive's score is not unique
    n_max = max(int(p.numel()) for p in pools)
    all_i, all_s = model.recommend(ep["seq_d1"][0], ep["seq_d2"][0], ep["domain_id"][0], k=n_max, pool=pools, exclude_history=False)
    all_i, all_s, pos = all_i.cpu(), all_s.cpu(), ep["i_node"].reshape(-1).cpu()
    left_out = 0
    for b in range(64):
        at = (all_i[b] == pos[b]).nonzero()
        assert at.numel() == 1, b                              # the positive is a member of its domain's pool
        if int((all_s[b] == all_s[b, at[0, 0]]).sum()) > 1:
            left_out += 1
            continue
        assert (int(pos[b]) in ids[b].tolist()) == (int(raw[b]) < k), (b, int(raw[b]))
    print(f"rows left out for a score tie with the positive: {left_out} of 64; rank_raw < {k} in {int((raw < k).sum())} rows")
    assert left_out <= 64 * 5 // 100
    assert 0 < int((raw < k).sum()) < 64                      # both sides of the equivalence occur


# ---- 6. command line -----------------------------------------------------------------------------------------------------------------------
def _write_csv(path, n, rng, lo1, hi1, lo2, hi2, ob_label=False):
    rows = ["user_id,seq_d1,seq_d2,domain_id" + (",ob_label" if ob_label else "")]
    for u in range(n):
        dom = int(rng.random() < 0.5)
        l1 = int(rng.integers(1 if dom == 0 else 0, 9))
        l2 = int(rng.integers(1 if dom == 1 else 0, 9))
        s1 = [int(x) for x in rng.integers(lo1, hi1, l1)]
        s2 = [int(x) for x in rng.integers(lo2, hi2, l2)]
        rows.append(f'{u},"{json.dumps(s1)}","{json.dumps(s2)}",{dom}' + (f",{int(rng.random() < 0.6)}" if ob_label else ""))
    with open(path, "w") as f:
        f.write("\n".join(rows) + "\n")


@pytest.mark.parametrize("model_name,emb", [("sasrec", "64"), ("bert4rec", "128")])
def test_cli_end_to_end(tmp_path, model_name, emb):
    from amid_amd import recommend, train_sr
    from amid_amd.dataset_seq import DeviceBatches, DualDomainSeqDataset
    rng = np.random.default_rng(0)
    root = tmp_path / "amazon_dataset"
    root.mkdir()
    _write_csv(root / "toy_train75.csv", 300, rng, 1, 400, 400, 900)
    _write_csv(root / "toy_test.csv", 80, rng, 1, 400, 400, 900)
    common = ["--data_root", str(tmp_path), "-ds", "amazon", "-dm", "toy", "--overlap_ratio", "0.75", "--model", model_name, "--bs", "32",
              "--seq_len", "20", "--emb_dim", emb, "--hid_dim", "16", "--neg_nums", "19"]
    train_sr.main(common + ["--epoch", "2", "--seeds", "1", "-md", str(tmp_path / "model"), "--save_dir", str(tmp_path / "run")])
    weights = str(tmp_path / "run" / "seed0" / "best_d1.pt")
    K = 10
    res = recommend.main(common + ["--weights", weights, "--topk", str(K), "--out", str(tmp_path / "top.npz"), "--metrics"])
    z = np.load(tmp_path / "top.npz")
    pad = 447410 + 1
    ds = DualDomainSeqDataset(seq_len=20, isTrain=False, neg_nums=19, long_length=7, pad_id=pad, seed=1000, csv_path=str(root / "toy_test.csv"))
    ds_train = DualDomainSeqDataset(seq_len=20, isTrain=True, neg_nums=1, long_length=7, pad_id=pad, seed=0, csv_path=str(root / "toy_train75.csv"))
    items, scores = z["items"], z["scores"]
    assert items.shape == (80, K) and scores.shape == (80, K) and items.dtype == np.int64 and scores.dtype == np.float32
    assert z["user_id"].tolist() == list(range(80)) and z["domain_id"].tolist() == ds.domain_id.tolist()      # every row, in CSV order
    assert np.array_equal(res["items"], items) and np.array_equal(res["scores"], scores)
    assert bool((scores[:, 1:] <= scores[:, :-1]).all())
    for r in range(80):
        d = int(ds.domain_id[r] != 0)
        assert set(items[r].tolist()) <= set(ds_train.pool[d].tolist()), r
        assert not set(items[r].tolist()) & set((ds.seq_d2 if d else ds.seq_d1)[r].tolist()), r
    # the same weights through model.recommend() on the same rows, in batches of 32 with the same fill
    args = recommend.build_parser().parse_args(common + ["--weights", weights])
    cls = {"sasrec": recommend.SASRec, "bert4rec": recommend.BERT4Rec}[model_name]
    model = cls(user_length=2 * 895510, user_emb_dim=int(emb), item_length=2 * 447410, item_emb_dim=int(emb), seq_len=20, hid_dim=16, bs=32,
                isInC=False, isItC=False, threshold1=0.5, threshold2=0.5, seed=0)
    assert recommend.load_weights(model, weights) == "state dict"
    model.eval()
    pools = tuple(torch.from_numpy(p).cuda() for p in ds_train.pool)
    sel = np.concatenate((np.arange(80), np.arange(16))).reshape(3, 32)
    want_i, want_s = [], []
    for rows in sel:
        i, s = model.recommend(torch.from_numpy(ds.seq_d1[rows]).cuda(), torch.from_numpy(ds.seq_d2[rows]).cuda(),
                               torch.from_numpy(ds.domain_id[rows]).cuda(), k=K, pool=pools)
        want_i.append(i.cpu().numpy())
        want_s.append(s.cpu().numpy())
    assert np.array_equal(np.concatenate(want_i)[:80], items) and np.array_equal(np.concatenate(want_s)[:80], scores)
    # --metrics: test()'s numbers for a model loaded with the same file
    want = train_sr.test(model, args, DeviceBatches(ds, 32, shuffle=False, device="cuda:0", seed=0))
    assert res["metrics"] == want


def test_cli_loads_a_training_state_and_the_full_history(tmp_path):
    """A last.pt is recognised by its format field; --history full recommends behind the held-out item, which then leaves the candidates."""
    from amid_amd import recommend, train_sr
    from amid_amd.dataset_seq import DualDomainSeqDataset
    rng = np.random.default_rng(1)
    root = tmp_path / "amazon_dataset"
    root.mkdir()
    _write_csv(root / "toy_train75.csv", 200, rng, 1, 400, 400, 900)
    _write_csv(root / "toy_test.csv", 40, rng, 1, 400, 400, 900)
    common = ["--data_root", str(tmp_path), "-ds", "amazon", "-dm", "toy", "--overlap_ratio", "0.75", "--model", "sasrec", "--bs", "32",
              "--seq_len", "20", "--emb_dim", "64", "--hid_dim", "16", "--neg_nums", "19"]
    train_sr.main(common + ["--epoch", "1", "--seeds", "1", "-md", str(tmp_path / "model"), "--save_dir", str(tmp_path / "run")])
    res = recommend.main(common + ["--weights", str(tmp_path / "run" / "seed0" / "last.pt"), "--topk", "256", "--pool", "table",
                                   "--history", "full", "--out", str(tmp_path / "top.npz")])
    ds = DualDomainSeqDataset(seq_len=20, isTrain=False, neg_nums=19, long_length=7, pad_id=447411, seed=1000, csv_path=str(root / "toy_test.csv"))
    assert res["items"].shape == (40, 256) and res["metrics"] is None
    for r in range(40):
        assert int(ds.i_node[r]) not in res["items"][r].tolist()
