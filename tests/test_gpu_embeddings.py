"""The encode / score split and the neighbour surface (SASRec.encode_users, recommend_from_vectors, neighbors, similar_items; recommend.py
--vectors_out / --similar_items) on plain SASRec, SASRec with isItC and with isDR at their bs rows, BERT4Rec and model_gru.GRU4Rec, on small
tables and short sequences.  ("sasrec", 70) is SASRec at D 64 beyond 64 tokens: the user vectors come from the forward's [2, B, D] there,
not from the fused evaluation.)"""
import numpy as np
import pytest
import torch

from tests.test_gpu_neighbors import check, reference
from tests.test_gpu_recommend_all import _model, _users, _write_csv

pytestmark = pytest.mark.gpu

KINDS = [("sasrec", 20), ("itc", 20), ("dr", 20), ("bert4rec", 20), ("gru4rec", 20), ("sasrec", 70)]


def make(kind, T, bs):
    if kind == "gru4rec":
        from tests.test_gpu_gru4rec import make_model
        m = make_model(120, T, 16, bs, seed=2)
        m.eval()
        return m
    return _model(kind, T, bs)


def own_history(users):
    return torch.where(users["domain_id"][..., None] != 0, users["seq_d2"], users["seq_d1"])


@pytest.mark.parametrize("kind,T", KINDS)
def test_encode_then_score_is_recommend_all(kind, T):
    n, B, k = 3, 8, 10
    model = make(kind, T, B)
    D = model.engine.D
    users = _users(n, B, T, seed=T + len(kind))
    pools = (torch.arange(1, 61, dtype=torch.int64).cuda(), torch.arange(40, 102, dtype=torch.int64).cuda())
    vec = model.encode_users(users, use_graph=True)
    eag = model.encode_users(users, use_graph=False)
    again = model.encode_users(users, use_graph=True)                  # the captured graph, replayed by a second call
    assert vec.shape == (n, B, D) and vec.dtype == torch.float32 and vec.is_cuda
    assert torch.equal(vec, eag) and torch.equal(vec, again)
    assert bool(torch.isfinite(vec).all()) and float(vec.abs().max()) > 0
    want_i, want_s = model.recommend_all(users, k=k, pool=pools)
    raw_i, raw_s = model.recommend_all(users, k=k, pool=pools, exclude_history=False)
    hist = own_history(users)
    for i in range(n):
        got_i, got_s = model.recommend_from_vectors(vec[i], users["domain_id"][i], k=k, pool=pools, history=hist[i])
        assert got_i.dtype == torch.int64 and got_s.dtype == torch.float32
        assert torch.equal(got_i, want_i[i]) and torch.equal(got_s, want_s[i]), i
        got_i, got_s = model.recommend_from_vectors(vec[i], users["domain_id"][i], k=k, pool=pools)
        assert torch.equal(got_i, raw_i[i]) and torch.equal(got_s, raw_s[i]), i
    # any B: the vectors are already mixed, so a comp model's bs does not bind the scorer
    flat_v, flat_d, flat_h = vec.reshape(-1, D), users["domain_id"].reshape(-1), hist.reshape(n * B, -1)
    for rows in (slice(0, 5), slice(3, 3 + 2 * B + 1)):
        got_i, got_s = model.recommend_from_vectors(flat_v[rows], flat_d[rows], k=k, pool=pools, history=flat_h[rows])
        assert torch.equal(got_i, want_i.reshape(n * B, k)[rows]) and torch.equal(got_s, want_s.reshape(n * B, k)[rows])
    # the whole table and a large k, as recommend() has them
    got_i, got_s = model.recommend_from_vectors(vec[0], users["domain_id"][0], k=256, history=hist[0])
    all_i, all_s = model.recommend_all(users, k=256)
    assert torch.equal(got_i, all_i[0]) and torch.equal(got_s, all_s[0])
    for bad in (0, 257):
        with pytest.raises(ValueError):
            model.recommend_from_vectors(vec[0], users["domain_id"][0], k=bad)
    with pytest.raises(ValueError):
        model.recommend_from_vectors(vec[0][:, :D - 1], users["domain_id"][0])
    if kind == "itc":
        with pytest.raises(ValueError):                               # the encoder keeps the comp models' "exactly bs rows" check
            model.encode_users({key: v[:, :5] for key, v in users.items()})


@pytest.mark.parametrize("kind,T", KINDS[:5])
def test_neighbours_of_items_and_of_users(kind, T):
    n, B = 3, 8
    model = make(kind, T, B)
    D = model.engine.D
    n_rows = model.engine.n_rows
    ids = torch.tensor([5, 1, 77, 30, 5, n_rows - 1], dtype=torch.int64).cuda()
    pool = torch.arange(1, 101, dtype=torch.int64).cuda()
    for metric in ("cosine", "dot"):
        for p in (None, pool):
            a_i, a_s = model.similar_items(ids, k=7, metric=metric, pool=p)
            b_i, b_s = model.neighbors(ids, base=None, k=7, metric=metric, pool=p, exclude_self=True)
            assert torch.equal(a_i, b_i) and torch.equal(a_s, b_s)
            assert a_i.shape == (6, 7) and not bool((a_i == ids[:, None]).any()) and bool((a_i >= 0).all())
            table = model.state_dict()["item_emb_layer.emb_item.weight"].detach().cpu().numpy()
            ref, bar = reference(table[ids.cpu().numpy()], table, metric)
            cands = np.arange(n_rows, dtype=np.int64) if p is None else p.cpu().numpy()
            check((kind, metric, "items"), a_i.cpu().numpy(), a_s.cpu().numpy(), ref, bar, cands, ids.cpu().tolist(), [], metric)
    # users like this user: stored encode_users output as the base
    users = _users(n, B, T, seed=3)
    vec = model.encode_users(users).reshape(-1, D).contiguous()
    x = vec.cpu().numpy()
    q = torch.arange(n * B, dtype=torch.int64).cuda()
    for metric in ("cosine", "dot"):
        i1, s1 = model.neighbors(q, base=vec, k=5, metric=metric)
        ref, bar = reference(x, x, metric)
        check((kind, metric, "users"), i1.cpu().numpy(), s1.cpu().numpy(), ref, bar, np.arange(n * B, dtype=np.int64), q.cpu().tolist(), [], metric)
        i2, s2 = model.neighbors(vec[:4], base=vec, k=5, metric=metric)      # vector queries: nothing to leave out
        check((kind, metric, "user vectors"), i2.cpu().numpy(), s2.cpu().numpy(), ref[:4], bar[:4], np.arange(n * B, dtype=np.int64), [-1] * 4,
              [], metric)
    with pytest.raises(ValueError):
        model.neighbors(q, base=vec, metric="l2")
    with pytest.raises(ValueError):
        model.neighbors(q, base=vec, k=257)
    with pytest.raises(ValueError):
        model.neighbors(q, base=vec[:, :32].contiguous())
    with pytest.raises(IndexError):
        model.similar_items(torch.tensor([3, n_rows], dtype=torch.int64).cuda(), k=3)
    model.similar_items(ids, k=3)                                      # (the flag does not outlive its IndexError)


def test_similar_items_chunks_its_queries():
    model = make("sasrec", 20, 8)
    ids = torch.arange(0, model.engine.n_rows, dtype=torch.int64).cuda()
    want = model.similar_items(ids, k=4)
    type(model).NEIGHBOR_CHUNK, keep = 17, type(model).NEIGHBOR_CHUNK
    try:
        got = model.similar_items(ids, k=4)
    finally:
        type(model).NEIGHBOR_CHUNK = keep
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.parametrize("kind", ["sasrec", "gru4rec"])
def test_similar_items_reads_the_flushed_table(kind):
    """A few train_steps leave rows with pending lazy-Adam steps; similar_items without an explicit flush reads the table as state_dict()
    gives it."""
    B, T = 8, 20
    model = make(kind, T, B)
    users = _users(3, B, T, seed=6)
    model.train()
    label = torch.zeros(B, 2, device="cuda")
    label[:, 0] = 1.0
    g = torch.Generator().manual_seed(1)
    for i in range(3):
        pos = torch.randint(1, 101, (B,), generator=g).cuda()
        neg = torch.randint(1, 101, (B, 1), generator=g).cuda()
        model.train_step(pos, neg, users["seq_d1"][i], users["seq_d2"][i], label, users["domain_id"][i])
    model.eval()
    ids = torch.arange(1, 101, dtype=torch.int64).cuda()
    got_i, got_s = model.similar_items(ids, k=6)
    table = model.state_dict()["item_emb_layer.emb_item.weight"].detach().clone().contiguous()
    want_i, want_s = model.neighbors(ids, base=table, k=6, exclude_self=True)
    assert torch.equal(got_i, want_i) and torch.equal(got_s, want_s)


def _cli_setup(tmp_path):
    from amid_amd import recommend
    rng = np.random.default_rng(0)
    root = tmp_path / "amazon_dataset"
    root.mkdir()
    _write_csv(root / "toy_train75.csv", 200, rng, 1, 400, 400, 900)
    _write_csv(root / "toy_test.csv", 40, rng, 1, 400, 400, 900)
    common = ["--data_root", str(tmp_path), "-ds", "amazon", "-dm", "toy", "--overlap_ratio", "0.75", "--model", "sasrec", "--bs", "32",
              "--seq_len", "20", "--emb_dim", "64", "--hid_dim", "16", "--neg_nums", "19"]
    model = recommend.SASRec(user_length=2 * 895510, user_emb_dim=64, item_length=2 * 447410, item_emb_dim=64, seq_len=20, hid_dim=16, bs=32,
                             isInC=False, isItC=False, threshold1=0.5, threshold2=0.5, seed=5)
    weights = str(tmp_path / "weights.pt")
    torch.save({k: v.detach().cpu() for k, v in model.state_dict().items()}, weights)
    model.eval()
    return recommend, root, common + ["--weights", weights], model


def test_cli_vectors_out_and_similar_items(tmp_path):
    from amid_amd.dataset_seq import DualDomainSeqDataset
    recommend, root, common, model = _cli_setup(tmp_path)
    K = 6
    plain = recommend.main(common + ["--topk", str(K), "--out", str(tmp_path / "plain.npz")])
    # --vectors_out: the rows encode_users returns, and --out untouched by the flag
    res = recommend.main(common + ["--topk", str(K), "--out", str(tmp_path / "top.npz"), "--vectors_out", str(tmp_path / "vec.npz")])
    a, b = np.load(tmp_path / "plain.npz"), np.load(tmp_path / "top.npz")
    assert sorted(a.files) == sorted(b.files) == ["domain_id", "items", "scores", "user_id"]              # the parent's file, key for key
    for key in a.files:
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), key
    assert sorted(plain) == ["domain_id", "items", "metrics", "scores", "user_id"]
    ds = DualDomainSeqDataset(seq_len=20, isTrain=False, neg_nums=19, long_length=7, pad_id=447411, seed=1000, csv_path=str(root / "toy_test.csv"))
    sel = recommend.filled_batches(40, 32)
    users = {"seq_d1": torch.from_numpy(ds.seq_d1[sel]).cuda(), "seq_d2": torch.from_numpy(ds.seq_d2[sel]).cuda(),
             "domain_id": torch.from_numpy(ds.domain_id[sel]).cuda()}
    want = model.encode_users(users).reshape(-1, 64)[:40].cpu().numpy()
    z = np.load(tmp_path / "vec.npz")
    assert sorted(z.files) == ["domain_id", "user_id", "vectors"]
    assert z["user_id"].tolist() == list(range(40)) and z["domain_id"].tolist() == ds.domain_id.tolist()
    assert z["vectors"].dtype == np.float32 and z["vectors"].tobytes() == want.tobytes() and np.array_equal(res["vectors"], want)
    ids, sc = model.recommend_all(users, k=K, pool=tuple(torch.from_numpy(p).cuda() for p in _train_pools(root)))
    assert np.array_equal(a["items"], ids.reshape(-1, K)[:40].cpu().numpy()) and np.array_equal(a["scores"], sc.reshape(-1, K)[:40].cpu().numpy())
    # --similar_items all: similar_items for the pools' items among the pools' items
    out = recommend.main(common + ["--topk", str(K), "--similar_items", "all", "--metric", "dot", "--out", str(tmp_path / "sim.npz")])
    s = np.load(tmp_path / "sim.npz")
    assert sorted(s.files) == ["item_id", "neighbors", "scores"]
    cand = torch.unique(torch.cat([torch.from_numpy(p).cuda() for p in _train_pools(root)]))
    w_i, w_s = model.similar_items(cand, k=K, metric="dot", pool=cand)
    assert np.array_equal(s["item_id"], cand.cpu().numpy()) and np.array_equal(s["neighbors"], w_i.cpu().numpy())
    assert s["scores"].tobytes() == w_s.cpu().numpy().tobytes() and np.array_equal(out["neighbors"], s["neighbors"])
    assert not (s["neighbors"] == s["item_id"][:, None]).any() and np.isin(s["neighbors"], s["item_id"]).all()
    # --similar_items FILE: the listed ids, cosine by default
    listed = cand[::7].cpu().numpy()
    (tmp_path / "ids.txt").write_text("\n".join(str(int(i)) for i in listed) + "\n")
    recommend.main(common + ["--topk", str(K), "--similar_items", str(tmp_path / "ids.txt"), "--out", str(tmp_path / "sim2.npz")])
    s2 = np.load(tmp_path / "sim2.npz")
    w_i, w_s = model.similar_items(torch.from_numpy(listed).cuda(), k=K, metric="cosine", pool=cand)
    assert np.array_equal(s2["item_id"], listed) and np.array_equal(s2["neighbors"], w_i.cpu().numpy())
    assert s2["scores"].tobytes() == w_s.cpu().numpy().tobytes()


def _train_pools(root):
    from amid_amd.dataset_seq import DualDomainSeqDataset
    ds_train = DualDomainSeqDataset(seq_len=20, isTrain=True, neg_nums=1, long_length=7, pad_id=447411, seed=0, csv_path=str(root / "toy_train75.csv"))
    return ds_train.pool
