"""Audience top-K (csrc/audience.hip, SasrecEngine.enqueue_audience_halves / enqueue_audience_topk, SASRec.recommend_users, recommend.py
--audience_of): for each item the k stored user vectors that score it highest, against the forward direction and against float64.

Models with random weights and no training; random finite vectors.  The expectation of a case is built ONCE from the forward direction:
recommend_from_vectors(V, vector_domain, k = pool size, pool = (the domain-0 query items, the domain-1 query items)) gives the dense score
matrix S[r, q]; the audience of q is the stable sort of its domain's rows by (score descending, row ascending), minus its holders.
recommend_users must return exactly those rows and bit-equal scores.

Shapes: N in {1, 255, 256, 257, 700, 2100} (the kernels' tile is 256 rows: one tile, the tile edge, several tiles), Q in {1, 8, 9, 40} (a
workgroup serves eight queries), k in {1, 10, 256}, D in {64, 128}, hid in {16, 32, 64}, vector domains all 0 / all 1 / mixed.  The top-K
launch cuts the tiles into ranges so as to fill 1024 workgroups, which at these sizes is a range per tile (the merge launch joins them);
every case above one tile runs again with the target lowered to 1 workgroup (one range walks every tile: the running lists and their
thresholds) and to 16 (2100 rows, 40 queries: ranges of several tiles, merged).

The independent statement (every case): p = sigmoid(w2 . relu((W1[:, :D] u + b1) + W1[:, D:] E[c]) + b2) from state_dict() in float64 on the
CPU.  Every returned score is within 2e-6 of it (the bar tests/test_gpu_eval.py holds the fused evaluation to against the oracle), and
every returned row's float64 score is at least the k-th best float64 score of its candidate set minus 4e-6 (twice that bar: the returned
row and the row it displaced may each be off by one bar)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NS = (1, 255, 256, 257, 700, 2100)
QS = (1, 8, 9, 40)
KS = (1, 10, 256)
LAYOUTS = ("zeros", "ones", "mixed")
BAR = 2e-6
_MODELS = {}


def model_of(kind, D, hid):
    key = (kind, D, hid)
    if key not in _MODELS:
        from amid_amd import model_gru, model_seq
        cls = {"sasrec": model_seq.SASRec, "bert4rec": model_seq.BERT4Rec, "gru4rec": model_gru.GRU4Rec}[kind]
        m = cls(10, D, 120, D, 20, hid, 8, False, False, 0.5, 0.3, seed=3)
        m.eval()
        _MODELS[key] = m
    return _MODELS[key]


def queries(n_rows, seed):
    """40 unique item ids with their domains (both domains among the first two, so that every prefix of two or more has both)."""
    rng = np.random.default_rng(seed)
    items = rng.permutation(np.arange(1, min(n_rows, 110)))[:40].astype(np.int64)
    dom = rng.integers(0, 2, 40).astype(np.int64)
    dom[0], dom[1] = 0, 1
    return items, dom


def domains(layout, N, seed):
    if layout == "zeros":
        return np.zeros(N, dtype=np.int64)
    if layout == "ones":
        return np.ones(N, dtype=np.int64)
    return np.random.default_rng(seed).integers(0, 2, N).astype(np.int64)


def forward_scores(model, V, vdom, items, dom):
    """S [N, Q] float32 (nan where the row's domain is not the query's) from recommend_from_vectors over the query items as the pools."""
    N, Q = V.shape[0], len(items)
    S = np.full((N, Q), np.nan, dtype=np.float32)
    pools = [np.sort(items[dom == d]) for d in (0, 1)]
    k = max(len(p) for p in pools)
    assert min(len(p) for p in pools) >= 1 and k <= 256 and len(set(zip(items.tolist(), dom.tolist()))) == Q
    ids, sc = model.recommend_from_vectors(V, torch.from_numpy(vdom).cuda(), k=k, pool=tuple(torch.from_numpy(p).cuda() for p in pools))
    ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
    for d in (0, 1):
        rows, n = np.nonzero((vdom != 0) == bool(d))[0], len(pools[d])
        col = np.array([int(np.nonzero((items == i) & (dom == d))[0][0]) for i in pools[d]])       # the pool entry's query
        got = ids[rows, :n]
        assert (got >= 0).all() and (ids[rows, n:] == -1).all() and (np.sort(got, axis=1) == pools[d][None, :]).all()
        S[rows[:, None], col[np.searchsorted(pools[d], got)]] = sc[rows, :n]
    return S


def float64_scores(model, V, items):
    """p [N, Q] of every (row, item) pair in float64 from state_dict() (the domains play no part in the formula)."""
    sd = {k: v.detach().cpu().double().numpy() for k, v in model.state_dict().items()}
    W1, b1 = sd["predictModule.fc.0.weight"], sd["predictModule.fc.0.bias"]
    w2, b2 = sd["predictModule.fc.2.weight"].reshape(-1), sd["predictModule.fc.2.bias"].reshape(-1)[0]
    D = V.shape[1]
    E = sd["item_emb_layer.emb_item.weight"][items]
    uh = V.cpu().double().numpy() @ W1[:, :D].T + b1                   # [N, hid]
    ih = E @ W1[:, D:].T                                               # [Q, hid]
    z = np.maximum(uh[:, None, :] + ih[None, :, :], 0.0) @ w2 + b2
    return 1.0 / (1.0 + np.exp(-z))


class Expect:
    """The expectation of one (vectors, domains, queries, holders) case, built once: per query its candidates by (forward score
    descending, row ascending) with those scores and their float64 scores; check() holds any (Q, k) against a prefix of it."""

    def __init__(self, S, P64, vdom, items, dom, removed=None):
        self.order = []
        for q in range(len(items)):
            cand = np.nonzero((vdom != 0) == (dom[q] != 0))[0]
            if removed is not None:
                cand = cand[~np.isin(cand, np.asarray(sorted(removed[q]), dtype=np.int64))]
            s = S[cand, q]
            assert not np.isnan(s).any()
            o = np.lexsort((cand, -s.astype(np.float64)))
            self.order.append((cand[o], s[o], P64[cand[o], q], np.sort(P64[cand, q])[::-1]))

    def check(self, tag, got_r, got_s, k):
        """Exact against the forward direction, and the float64 statement, for every query of the call (the first len(got_r))."""
        for q in range(len(got_r)):
            rows, sc, p, p_desc = self.order[q]
            n = min(k, len(rows))
            assert np.array_equal(got_r[q][:n], rows[:n]) and (got_r[q][n:] == -1).all(), (tag, q, got_r[q][:12], rows[:12])
            assert got_s[q][:n].tobytes() == sc[:n].tobytes() and np.isneginf(got_s[q][n:]).all(), (tag, q)
            if n == 0:
                continue
            err = np.abs(got_s[q][:n].astype(np.float64) - p[:n])
            assert (err <= BAR).all(), (tag, q, float(err.max()))
            assert (p[:n] >= p_desc[n - 1] - 2 * BAR).all(), (tag, q, float((p_desc[n - 1] - p[:n]).max()))


def run(model, items, dom, V, vdom, k, holders=None, wgs=0):
    """wgs: the top-K launch's target workgroup count for this call (0: the default, 1024 -- at these sizes a range per tile; 1: one range
    walks every tile, the running lists and their thresholds at work; 16 with 40 queries: ranges of several tiles, merged)."""
    from amid_amd._lib import lib
    lib().value("amid_audience_target_workgroups", wgs)
    try:
        r, s = model.recommend_users(torch.from_numpy(items).cuda(), torch.from_numpy(dom).cuda(), V, torch.from_numpy(vdom).cuda(), k=k,
                                     holders=holders)
    finally:
        lib().value("amid_audience_target_workgroups", 0)
    assert r.dtype == torch.int64 and s.dtype == torch.float32 and r.shape == (len(items), k) and s.shape == (len(items), k) and r.is_cuda
    return r.cpu().numpy(), s.cpu().numpy()


def vectors(N, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, D, generator=g).cuda().contiguous()


# ---- 1. and 4.: exact against the forward direction, and against float64 ----------------------------------------------------------------------
@pytest.mark.parametrize("hid", (16, 32, 64))
@pytest.mark.parametrize("D", (64, 128))
def test_audience_is_the_forward_scores_sorted(D, hid):
    model = model_of("sasrec", D, hid)
    items, dom = queries(model.engine.n_rows, seed=D + hid)
    for N in NS:
        V = vectors(N, D, seed=N + hid)
        P64 = float64_scores(model, V, items)
        for layout in LAYOUTS:
            vdom = domains(layout, N, seed=N)
            exp = Expect(forward_scores(model, V, vdom, items, dom), P64, vdom, items, dom)
            for Q in QS:
                for k in KS:
                    for wgs in ((0,) if N <= 256 else (0, 1, 16)):
                        got_r, got_s = run(model, items[:Q], dom[:Q], V, vdom, k, wgs=wgs)
                        exp.check((D, hid, N, layout, Q, k, wgs), got_r, got_s, k)
                        if layout != "mixed":                          # queries of the empty domain: all padding
                            empty = (dom[:Q] != 0) != (layout == "ones")
                            assert (got_r[empty] == -1).all() and np.isneginf(got_s[empty]).all()


def test_the_queries_go_in_chunks():
    model = model_of("sasrec", 64, 16)
    items, dom = queries(model.engine.n_rows, seed=5)
    V, vdom = vectors(700, 64, seed=9), domains("mixed", 700, seed=9)
    hold = (torch.arange(0, 700, 3).repeat(40), torch.arange(41) * len(range(0, 700, 3)))
    want = run(model, items, dom, V, vdom, 10, holders=hold)
    eng = model.engine
    eng.AUDIENCE_CHUNK = 7
    try:
        got = run(model, items, dom, V, vdom, 10, holders=hold)
        with pytest.raises(ValueError):
            eng.enqueue_audience_topk(torch.from_numpy(items).cuda(), torch.from_numpy(dom).cuda(),
                                      (torch.zeros(1, dtype=torch.int32).cuda(), torch.zeros(0, dtype=torch.int32).cuda()), None, 3,
                                      torch.zeros(40, 3, dtype=torch.int64).cuda(), torch.zeros(40, 3).cuda(), eng.flags_holder().err)
    finally:
        del eng.AUDIENCE_CHUNK
    assert np.array_equal(got[0], want[0]) and got[1].tobytes() == want[1].tobytes()
    assert not np.isin(want[0], np.arange(0, 700, 3)).any()


# ---- 2. ties ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (64, 128))
def test_ties_go_to_the_lower_row(D):
    """Bit-identical vectors in one tile (rows 3, 4) and in another (row 300): equal score bits, the lower row first, and a k that cuts
    through the group keeps the lower rows."""
    model = model_of("sasrec", D, 32)
    items, dom = queries(model.engine.n_rows, seed=1)
    N = 310
    V = vectors(N, D, seed=2)
    V[4] = V[3]
    V[300] = V[3]
    vdom = np.zeros(N, dtype=np.int64)
    exp = Expect(forward_scores(model, V, vdom, items, dom), float64_scores(model, V, items), vdom, items, dom)
    got_r, got_s = run(model, items, dom, V, vdom, 256)
    exp.check(("ties", D), got_r, got_s, 256)
    one_r, one_s = run(model, items, dom, V, vdom, 256, wgs=1)         # ... and with both tiles in one range
    assert np.array_equal(one_r, got_r) and one_s.tobytes() == got_s.tobytes()
    cut = 0
    for q in np.nonzero(dom == 0)[0]:
        pos = {int(r): i for i, r in enumerate(got_r[q])}
        if 3 not in pos or pos[3] > 253:
            continue
        p = pos[3]
        assert got_r[q][p:p + 3].tolist() == [3, 4, 300] and got_s[q][p] == got_s[q][p + 1] == got_s[q][p + 2]
        assert got_s[q][p:p + 3].tobytes() == got_s[q][p:p + 1].tobytes() * 3
        for k in (p + 1, p + 2):
            if cut >= 6:
                break
            r_k, s_k = run(model, items[q:q + 1], dom[q:q + 1], V, vdom, k)
            assert r_k[0].tolist() == got_r[q][:k].tolist() and r_k[0][p:].tolist() == [3, 4, 300][:k - p]
            assert s_k[0].tobytes() == got_s[q][:k].tobytes()
            cut += 1
    assert cut >= 2


# ---- 3. holders -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (10, 256))
def test_holders_are_left_out(k):
    D, N, Q = 64, 700, 9
    model = model_of("sasrec", D, 32)
    items, dom = queries(model.engine.n_rows, seed=4)
    V, vdom = vectors(N, D, seed=6), domains("mixed", N, seed=6)
    S, P64 = forward_scores(model, V, vdom, items, dom)[:, :Q], float64_scores(model, V, items[:Q])
    items, dom = items[:Q], dom[:Q]
    plain_r, _ = run(model, items, dom, V, vdom, k)
    own = lambda q: np.nonzero((vdom != 0) == (dom[q] != 0))[0]        # noqa: E731
    other = lambda q: np.nonzero((vdom != 0) != (dom[q] != 0))[0]      # noqa: E731
    lists = [
        [int(plain_r[0][0])],                                          # the top row of the query
        own(1).tolist(),                                               # every candidate: all padding
        list(range(0, N, 3)),                                          # several tiles, both domains' rows among them
        [5, 5, 600, 2, 300, 2, 699, 0],                                # duplicates, unsorted
        [-3, N, N + 50, 2 ** 40, int(plain_r[4][1]), -1],              # out of range around one real entry
        other(5).tolist(),                                             # only rows of the other domain: nothing leaves
        [],
        plain_r[7][:min(k, 5)].tolist()[::-1],                         # its best five, descending
        own(8)[::2].tolist() + own(8)[::2].tolist(),                   # every second candidate, twice
    ]
    idx = torch.tensor([x for li in lists for x in li], dtype=torch.int64)
    off = torch.tensor(np.concatenate(([0], np.cumsum([len(li) for li in lists]))), dtype=torch.int64)
    exp = Expect(S, P64, vdom, items, dom, removed=[set(li) for li in lists])
    for wgs in (0, 1):
        got_r, got_s = run(model, items, dom, V, vdom, k, holders=(idx.cuda(), off.cuda()), wgs=wgs)
        exp.check(("holders", k, wgs), got_r, got_s, k)
    assert int(plain_r[0][0]) not in got_r[0] and (got_r[1] == -1).all() and np.isneginf(got_s[1]).all()
    assert np.array_equal(got_r[5], plain_r[5]) and np.array_equal(got_r[6], plain_r[6])
    # host lists and numpy arrays are taken as well
    again_r, again_s = run(model, items, dom, V, vdom, k, holders=(idx.numpy(), off.tolist()))
    assert np.array_equal(again_r, got_r) and again_s.tobytes() == got_s.tobytes()


# ---- 5. the inherited method on the other models ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,D", [("gru4rec", 128), ("bert4rec", 128)])
def test_gru4rec_and_bert4rec_inherit_it(kind, D):
    model = model_of(kind, D, 16)
    items, dom = queries(model.engine.n_rows, seed=8)
    N, k = 700, 10
    V, vdom = vectors(N, D, seed=12), domains("mixed", N, seed=12)
    exp = Expect(forward_scores(model, V, vdom, items, dom), float64_scores(model, V, items), vdom, items, dom)
    got_r, got_s = run(model, items, dom, V, vdom, k)
    exp.check((kind,), got_r, got_s, k)


# ---- 6. the index flag and the argument checks --------------------------------------------------------------------------------------------------
def test_an_item_outside_the_table_raises():
    model = model_of("sasrec", 64, 16)
    n_rows = model.engine.n_rows
    items, dom = queries(n_rows, seed=3)
    V, vdom = vectors(300, 64, seed=1), domains("mixed", 300, seed=1)
    for bad_id in (n_rows, n_rows + 7, -1):
        bad = items[:9].copy()
        bad[4] = bad_id
        with pytest.raises(IndexError):
            run(model, bad, dom[:9], V, vdom, 5)
    good_r, good_s = run(model, items[:9], dom[:9], V, vdom, 5)        # (the flag does not outlive its IndexError)
    Expect(forward_scores(model, V, vdom, items, dom), float64_scores(model, V, items), vdom, items, dom).check(("clean",), good_r, good_s, 5)


def test_bad_arguments_raise_value_error():
    model = model_of("sasrec", 64, 16)
    items, dom = queries(model.engine.n_rows, seed=3)
    it, dm = torch.from_numpy(items[:4]).cuda(), torch.from_numpy(dom[:4]).cuda()
    V, vdom = vectors(30, 64, seed=1), torch.zeros(30, dtype=torch.int64).cuda()
    for k in (0, 257):
        with pytest.raises(ValueError):
            model.recommend_users(it, dm, V, vdom, k=k)
    for bad_v in (V[:, :32].contiguous(), V.cpu(), V.double(), V.t().contiguous().t(), V[:0]):
        with pytest.raises(ValueError):
            model.recommend_users(it, dm, bad_v, vdom[:bad_v.shape[0]])
    with pytest.raises(ValueError):
        model.recommend_users(it, dm, V, vdom[:7])
    with pytest.raises(ValueError):
        model.recommend_users(it, dm[:3], V, vdom)
    with pytest.raises(ValueError):
        model.recommend_users(it[:0], dm[:0], V, vdom)
    for bad_h in ((torch.tensor([1, 2]), torch.tensor([0, 1, 2])), (torch.tensor([1, 2]), torch.tensor([0, 1, 1, 1, 3])),
                  (torch.tensor([1, 2]), torch.tensor([0, 2, 1, 2, 2])), (torch.tensor([1, 2]), torch.tensor([1, 1, 1, 2, 2])), torch.tensor([1])):
        with pytest.raises(ValueError):
            model.recommend_users(it, dm, V, vdom, holders=bad_h)


# ---- 7. the command line ----------------------------------------------------------------------------------------------------------------------
def test_cli_audience_of(tmp_path):
    from amid_amd.dataset_seq import DualDomainSeqDataset
    from tests.test_gpu_embeddings import _cli_setup, _train_pools
    recommend, root, common, model = _cli_setup(tmp_path)
    K = 5
    out = recommend.main(common + ["--topk", str(K), "--audience_of", "all", "--out", str(tmp_path / "aud.npz"),
                                   "--vectors_out", str(tmp_path / "vec.npz")])
    z = np.load(tmp_path / "aud.npz")
    assert sorted(z.files) == ["domain_id", "item_id", "rows", "scores", "users"]
    ds = DualDomainSeqDataset(seq_len=20, isTrain=False, neg_nums=19, long_length=7, pad_id=447411, seed=1000, csv_path=str(root / "toy_test.csv"))
    sel = recommend.filled_batches(40, 32)
    users = {"seq_d1": torch.from_numpy(ds.seq_d1[sel]).cuda(), "seq_d2": torch.from_numpy(ds.seq_d2[sel]).cuda(),
             "domain_id": torch.from_numpy(ds.domain_id[sel]).cuda()}
    vec = model.encode_users(users).reshape(-1, 64)[:40].contiguous()
    pools = _train_pools(root)
    items = np.concatenate(pools).astype(np.int64)
    dom = np.concatenate((np.zeros(len(pools[0]), dtype=np.int64), np.ones(len(pools[1]), dtype=np.int64)))
    want_r, want_s = run(model, items, dom, vec, ds.domain_id.astype(np.int64), K)
    assert np.array_equal(z["item_id"], items) and np.array_equal(z["domain_id"], dom)
    assert np.array_equal(z["rows"], want_r) and z["scores"].tobytes() == want_s.tobytes() and z["scores"].dtype == np.float32
    assert np.array_equal(z["users"], np.where(want_r >= 0, ds.user_nodes[np.maximum(want_r, 0)], -1)) and np.array_equal(out["rows"], want_r)
    assert (want_r >= 0).any() and ((ds.domain_id[np.maximum(want_r, 0)] != 0) == (dom[:, None] != 0))[want_r >= 0].all()
    # --vectors_in on the file --vectors_out wrote: the same file
    recommend.main(common + ["--topk", str(K), "--audience_of", "all", "--out", str(tmp_path / "aud2.npz"), "--vectors_in", str(tmp_path / "vec.npz")])
    z2 = np.load(tmp_path / "aud2.npz")
    for key in z.files:
        assert z[key].dtype == z2[key].dtype and z[key].shape == z2[key].shape and z[key].tobytes() == z2[key].tobytes(), key
    # --exclude_holders removes exactly the holders: rows whose own-domain history or held-out item is the item
    recommend.main(common + ["--topk", str(K), "--audience_of", "all", "--exclude_holders", "--out", str(tmp_path / "aud3.npz"),
                             "--vectors_in", str(tmp_path / "vec.npz")])
    z3 = np.load(tmp_path / "aud3.npz")
    lists, n_held = [], 0
    for i, d in zip(items, dom):
        own = np.concatenate(((ds.seq_d2 if d else ds.seq_d1), ds.i_node[:, None]), axis=1)
        li = np.nonzero(((ds.domain_id != 0) == bool(d)) & (own == i).any(axis=1))[0].tolist()
        n_held += len(li)
        lists.append(li)
    assert n_held > 0
    idx = torch.tensor([x for li in lists for x in li], dtype=torch.int64)
    off = torch.tensor(np.concatenate(([0], np.cumsum([len(li) for li in lists]))), dtype=torch.int64)
    held_r, held_s = run(model, items, dom, vec, ds.domain_id.astype(np.int64), K, holders=(idx, off))
    assert np.array_equal(z3["rows"], held_r) and z3["scores"].tobytes() == held_s.tobytes()
    full_r, _ = run(model, items, dom, vec, ds.domain_id.astype(np.int64), 40)
    for q, li in enumerate(lists):                                     # the unexcluded order with the holders struck out
        keep = [int(r) for r in full_r[q] if r >= 0 and int(r) not in set(li)]
        assert z3["rows"][q].tolist() == (keep + [-1] * K)[:K], q
    # a FILE of "item_id domain_id" pairs
    pick = np.stack((items[::9], dom[::9]), axis=1)
    (tmp_path / "pairs.txt").write_text("\n".join(f"{int(i)} {int(d)}" for i, d in pick) + "\n")
    recommend.main(common + ["--topk", str(K), "--audience_of", str(tmp_path / "pairs.txt"), "--out", str(tmp_path / "aud4.npz")])
    z4 = np.load(tmp_path / "aud4.npz")
    assert np.array_equal(z4["item_id"], pick[:, 0]) and np.array_equal(z4["rows"], want_r[::9]) and z4["scores"].tobytes() == want_s[::9].tobytes()
    # a vectors file that is not this CSV's: another row count, another user_id column
    v = np.load(tmp_path / "vec.npz")
    np.savez(tmp_path / "short.npz", user_id=v["user_id"][:-1], domain_id=v["domain_id"][:-1], vectors=v["vectors"][:-1])
    np.savez(tmp_path / "other.npz", user_id=v["user_id"][::-1].copy(), domain_id=v["domain_id"], vectors=v["vectors"])
    for name in ("short.npz", "other.npz"):
        with pytest.raises(SystemExit) as e:
            recommend.main(common + ["--topk", str(K), "--audience_of", "all", "--out", str(tmp_path / "no.npz"), "--vectors_in", str(tmp_path / name)])
        assert "does not match the users CSV" in str(e.value)
    assert not (tmp_path / "no.npz").exists()
    with pytest.raises(SystemExit):                                    # a joint job is refused, as for the other modes
        recommend.main([a if a != "toy" else "toy+toy" for a in common] + ["--audience_of", "all"])
