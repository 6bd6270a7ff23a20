"""Diversified top-K (csrc/diversify.hip, SasrecEngine.enqueue_mmr_lists, SASRec.diversify / recommend_diverse, recommend.py --diversify)
against the float64 restatement tests/mmr_ref.py and, bit for bit, against the paths it is built from.

Shapes: a table of 600 rows, D 64 / 128, B in {1, 3, 17}, list lengths {0, 1, 2, K - 1, K, 40, 257, 600} mixed within one call (257 and 600
are two and three tiles of 256 entries: the units' lists are merged), shortlist in {K, 16, 256}, K in {1, 5, 16}, one case of K = shortlist =
256 at D 128, both metrics, lambda in {0, 0.3, 0.7, 1}.  Every raw call writes into guarded allocations (a sentinel before and after, NaN or a
marker inside, the workspace included).

1. Exact flavour.  Table entries are small integers / 8, relevances multiples of 1 / 64, lambda 0.5, the metric dot: every fp32 operation
   of the kernel is exact, so ids, positions, relevances, values and max_sims must EQUAL the float64 restatement -- with bit-equal table rows
   (exact ties of the criterion), repeated ids, ids outside the table (flag raised) and NaN relevances planted.

2. Plain flavour.  A randn table and the scorer's real relevance (rank_candidates_from_vectors' list_scores).  The bound on v and on max_sim
   is mmr_ref's, derived in its docstring from the order of operations csrc/diversify.hip and csrc/sim_parts.h document: one fmaf chain of D
   terms from 0 for the dot product (gamma_D sum |a_i b_i|); for the cosine the two inverse norms, each eight fmaf chains of D / 8 squares
   joined by three levels of additions, a square root and a division (relative rho = gamma_(D/8+3) / 2 + 4 u), and two multiplications;
   the running maximum moves by at most the largest perturbation of its arguments; v = fl(fl(lam rel) - fl(oml m)) adds
   2 u (|lam rel| + |oml m|).  Per entry, from the float64 operands; nothing fitted.  The seeds below were chosen on the CPU so that at
   every greedy step of every row the best value leads EVERY other candidate by more than the sum of the two entries' bounds, and the
   runner-up by more than twice the larger bound; the test asserts that itself in float64 before it looks at the kernel's result.  Then the
   picks must be the restatement's at every step and values / max_sims within the bound.  The worst |error| / bound per metric and D goes to
   the parity log (profiles/diversify.md); a ratio above 1 means the kernel or the derivation is wrong.

3. Bit ties to what exists: lam = 1 is rank_candidates_from_vectors' top-K; max_sims[:, 1] is neighbors' score of (pick 2, pick 1);
   recommend_diverse is recommend(k = shortlist) followed by diversify; a row alone equals the row in a batch of 17; chunks of 2 rows / 64
   entries change nothing.

4. recommend.py --diversify in both modes on a toy dataset."""
import numpy as np
import pytest
import torch

from tests import mmr_ref
from tests.test_gpu_sasrec import log

pytestmark = pytest.mark.gpu

N_ITEMS = 600
GUARD = 2048
SENT = -12345.625                # guard value: exact in float32, far from every output
MARK = -(2 ** 62)                # "never written" inside an int64 output
FIELDS = ("ids", "rel", "value", "max_sim", "positions")
_MODELS, _WORST = {}, {}


# ---- guarded raw calls ------------------------------------------------------------------------------------------------------------------------------
class Guarded:
    """n elements inside a larger allocation: NaN (floats) / MARK (int64) / 0xEE (bytes) inside, the sentinel before and after."""

    def __init__(self, n, dtype):
        self.n, self.dtype = n, dtype
        self.sent = {torch.float32: SENT, torch.int64: -12345, torch.uint8: 0xA5}[dtype]
        self.buf = torch.full((GUARD + n + GUARD,), self.sent, dtype=dtype, device="cuda")
        self.t = self.buf[GUARD:GUARD + n]
        self.t.fill_({torch.float32: float("nan"), torch.int64: MARK, torch.uint8: 0xEE}[dtype])

    def cpu(self, tag):
        b = self.buf.cpu()
        assert bool((b[:GUARD] == self.sent).all()) and bool((b[GUARD + self.n:] == self.sent).all()), f"{tag}: a write outside the allocation"
        o = b[GUARD:GUARD + self.n].clone()
        if self.dtype == torch.float32:
            assert not bool(torch.isnan(o).any()), f"{tag}: an element was not written"
        elif self.dtype == torch.int64:
            assert not bool((o == MARK).any()), f"{tag}: an element was not written"
        return o


def run_raw(items, off, rel, table, metric, lam, K, M):
    """amid_mmr_lists_f32 through the C ABI on torch's stream, every output and the workspace guarded.  Returns ({field: CPU [B, K]}, flags)."""
    from amid_amd._lib import lib
    items = torch.as_tensor(items, dtype=torch.int64).cuda().contiguous()
    off = torch.as_tensor(off, dtype=torch.int64).cuda().contiguous()
    rel = torch.as_tensor(rel, dtype=torch.float32).cuda().contiguous()
    B, n = off.numel() - 1, items.numel()
    n_rows, D = table.shape
    nbytes = int(lib().value("amid_mmr_workspace_bytes", B, n, D, K, M))
    assert nbytes > 0
    ws = Guarded(nbytes, torch.uint8)
    outs = [Guarded(B * K, torch.int64 if f in ("ids", "positions") else torch.float32) for f in FIELDS]
    flags = torch.zeros(1, dtype=torch.int32, device="cuda")
    ptr = lambda t: None if t.numel() == 0 else t.data_ptr()          # noqa: E731
    lib().call("amid_mmr_lists_f32", ptr(items), off.data_ptr(), ptr(rel), n, B, table.data_ptr(), n_rows, D, metric, float(lam), K, M,
               ws.t.data_ptr(), flags.data_ptr(), *(o.t.data_ptr() for o in outs), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    tag = (B, n, D, metric, lam, K, M)
    ws.cpu(tag)
    return {f: o.cpu((tag, f)).reshape(B, K) for f, o in zip(FIELDS, outs)}, int(flags.item())


def csr(lists):
    off = np.concatenate(([0], np.cumsum([len(li) for li in lists]))).astype(np.int64)
    items = np.concatenate([np.asarray(li, dtype=np.int64) for li in lists]) if off[-1] else np.zeros(0, dtype=np.int64)
    return torch.from_numpy(items), torch.from_numpy(off)


def lens_for(B, K, shift=0):
    """B list lengths out of {0, 1, 2, K - 1, K, 40, 257, 600}, the long ones first so that every B sees two tiles and three."""
    pool = (600, 257, 0, K, 40, 1, K - 1, 2)
    return [pool[(b + shift) % len(pool)] for b in range(B)]


def same_picks(tag, got, want):
    B = len(want)
    for f in ("ids", "positions"):
        w = mmr_ref.stack(want, f, torch.int64)
        assert torch.equal(got[f], w), (tag, f, [(b, got[f][b].tolist()[:8], w[b].tolist()[:8]) for b in range(B) if not torch.equal(got[f][b], w[b])][:2])
    w = mmr_ref.stack(want, "rel", torch.float64)
    assert torch.equal(got["rel"].to(torch.float64), w), (tag, "rel")


# ---- 1. the exact flavour -----------------------------------------------------------------------------------------------------------------------------
def exact_inputs(D, lens, seed, bad):
    g = torch.Generator().manual_seed(seed)
    table = torch.randint(-4, 5, (N_ITEMS, D), generator=g).to(torch.float32) / 8
    table[100:110] = table[7]                                           # bit-equal rows: equal similarities, equal criteria
    table[300] = 0.0                                                    # a zero row
    lists, rels = [], []
    for n in lens:
        ids = torch.randint(0, N_ITEMS, (n,), generator=g)
        if n >= 40:
            ids[torch.randperm(n, generator=g)[:12]] = torch.tensor([7, 100, 101, 102, 103, 104, 105, 300, 7, 100, 101, 300])
            ids[n // 2] = ids[0]                                        # a repeated id among the rest
        r = torch.randint(0, 33, (n,), generator=g).to(torch.float32) / 64
        if n >= 40:
            r[ids == 7] = 1.0                                           # the planted rows lead the shortlist: their ties are reached
            r[(ids >= 100) & (ids < 110)] = 1.0 - 1.0 / 64
        if bad and n >= 2:
            at = torch.randperm(n, generator=g)[:max(1, n // 10)]
            ids[at[0::3]] = -1
            ids[at[1::3]] = N_ITEMS
            r[at[1::3]] = 2.0                                           # (the best relevance of the list on an id outside the table)
            r[at[2::3]] = float("nan")
            if n >= 40:
                ids[1] = 1 << 40
        lists.append(ids.numpy())
        rels.append(r)
    return table, lists, torch.cat(rels) if lens else torch.zeros(0)


@pytest.mark.parametrize("D", (64, 128))
def test_exact_flavour_equals_the_restatement(D):
    seed = 0
    for K in (1, 5, 16):
        for M in sorted({K, 16, 256}):
            for B in (1, 3, 17):
                for bad in (False, True):
                    seed += 1
                    lens = lens_for(B, K, shift=seed)
                    table, lists, rel = exact_inputs(D, lens, seed, bad)
                    items, off = csr(lists)
                    got, flags = run_raw(items, off, rel, table.cuda(), 0, 0.5, K, M)
                    want = mmr_ref.mmr_lists(items, off, rel, table, 0, 0.5, K, M)
                    tag = ("exact", D, K, M, B, bad, lens)
                    same_picks(tag, got, want)
                    for f in ("value", "max_sim"):
                        assert torch.equal(got[f].to(torch.float64), mmr_ref.stack(want, f, torch.float64)), (tag, f)
                    has_bad = bool(((items < 0) | (items >= N_ITEMS)).any())
                    assert flags == (1 if has_bad else 0), (tag, flags)
                    assert bad == has_bad or max(lens) < 2


def test_exact_flavour_at_k_256():
    table, lists, rel = exact_inputs(128, [600, 257, 300], 99, True)
    items, off = csr(lists)
    got, flags = run_raw(items, off, rel, table.cuda(), 0, 0.5, 256, 256)
    want = mmr_ref.mmr_lists(items, off, rel, table, 0, 0.5, 256, 256)
    same_picks(("exact 256",), got, want)
    for f in ("value", "max_sim"):
        assert torch.equal(got[f].to(torch.float64), mmr_ref.stack(want, f, torch.float64)), f
    assert flags == 1 and (got["ids"][0] >= 0).sum() > 150 and (got["ids"][:, -1] == -1).all()      # (repeated ids: fewer than 256 picks)


# ---- 2. the plain flavour -----------------------------------------------------------------------------------------------------------------------------
def model_of(D, kind="sasrec"):
    """A model with random weights over a randn table of N_ITEMS rows."""
    key = (kind, D)
    if key not in _MODELS:
        from amid_amd import model_gru, model_seq
        cls = {"sasrec": model_seq.SASRec, "bert4rec": model_seq.BERT4Rec, "gru4rec": model_gru.GRU4Rec}[kind]
        m = cls(10, D, N_ITEMS, D, 20, 16, 8, False, False, 0.5, 0.3, seed=3)
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        g = torch.Generator().manual_seed(1000 + D)
        sd["item_emb_layer.emb_item.weight"] = torch.randn(tuple(sd["item_emb_layer.emb_item.weight"].shape), generator=g)
        m.load_state_dict(sd)
        m.eval()
        _MODELS[key] = m
    return _MODELS[key]


def plain_inputs(D, lens, seed):
    """Lists of distinct ids per row (a list of 600: every id of the table, in random order), random vectors, and the scorer's relevance of
    every entry."""
    model = model_of(D)
    rng = np.random.default_rng(seed)
    lists = [rng.permutation(N_ITEMS)[:n].astype(np.int64) for n in lens]
    g = torch.Generator().manual_seed(seed)
    V = torch.randn(len(lens), D, generator=g).cuda()
    dom = torch.arange(len(lens)) % 2
    items, off = csr(lists)
    rel = model.rank_candidates_from_vectors(V, dom, (items, off), k=None, list_scores=True).list_scores
    return model, V, dom, items, off, rel.cpu()


# (name, D, B, the lengths or None for lens_for, K, shortlist, metric, lambda, seed)
PLAIN = [
    ("17 rows cosine", 64, 17, None, 5, 16, 1, 0.7, 0),
    ("17 rows dot wide", 128, 17, None, 16, 256, 0, 0.3, 1),
    ("k 1", 64, 3, (40, 600, 0), 1, 1, 1, 0.0, 0),
    ("shortlist = k, lam 1", 128, 1, (257,), 5, 5, 0, 1.0, 0),
    ("k = shortlist = 256", 128, 1, (600,), 256, 256, 1, 0.7, 19),
    ("17 rows dot", 64, 17, None, 16, 16, 0, 0.7, 0),
    ("3 rows cosine wide", 128, 3, (600, 2, 257), 5, 256, 1, 0.3, 0),
    ("lam 0", 64, 1, (600,), 16, 256, 1, 0.0, 0),
    ("k = shortlist = 256 dot", 128, 1, (257,), 256, 256, 0, 0.3, 105),
]


def plain_case(case):
    name, D, B, lens, K, M, metric, lam, seed = case
    lens = lens_for(B, K) if lens is None else list(lens)
    model, V, dom, items, off, rel = plain_inputs(D, lens, seed)
    want = mmr_ref.mmr_lists(items, off, rel, model.engine.table.cpu(), metric, lam, K, M, with_bound=True)
    margins = [mg for row in want for mg in row["margins"]]
    return model, items, off, rel, want, margins


@pytest.mark.parametrize("case", PLAIN, ids=[c[0] for c in PLAIN])
def test_plain_flavour_within_the_derived_bound(case):
    name, D, B, lens, K, M, metric, lam, seed = case
    model, items, off, rel, want, margins = plain_case(case)
    # the restatement's picks are decided beyond what fp32 can move: asserted before the kernel's result is looked at
    worst_margin = min((min(a, b) for a, b in margins), default=1.0)
    print(f"{name}: {len(margins)} greedy steps, the smallest margin over the bound {worst_margin:.3e}")
    assert worst_margin > 0, (name, seed, worst_margin)
    got, flags = run_raw(items, off, rel, model.engine.table, metric, lam, K, M)
    assert flags == 0
    same_picks(("plain", name), got, want)
    ratio = 0.0
    for f, e in (("value", "e_value"), ("max_sim", "e_max_sim")):
        w, bound = mmr_ref.stack(want, f, torch.float64), mmr_ref.stack(want, e, torch.float64)
        some = torch.isfinite(w)
        assert torch.equal(got[f][~some].to(torch.float64), w[~some]), (name, f, "padding")
        err = (got[f].to(torch.float64) - w)[some].abs()
        r = float((err / bound[some].clamp(min=1e-300)).max()) if err.numel() and float(err.max()) > 0 else 0.0
        print(f"{name}: {f} worst |error| {float(err.max()) if err.numel() else 0.0:.3e}, worst |error| / bound {r:.3f}")
        log(f"diversify {name} D {D} metric {metric} lam {lam} K {K} M {M}: {f} worst |err| {float(err.max()) if err.numel() else 0.0:.3e} ratio {r:.3f}")
        assert bool((err <= bound[some]).all()), (name, f, r)
        ratio = max(ratio, r)
    key = (("dot", "cosine")[metric], D)
    _WORST[key] = max(_WORST.get(key, 0.0), ratio)
    log(f"diversify worst |error| / bound so far {key}: {_WORST[key]:.3f}")


# ---- 3. bit ties to what exists -------------------------------------------------------------------------------------------------------------------------
def bits(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize("D", (64, 128))
def test_lam_1_is_the_ranked_list_and_max_sim_is_neighbors_score(D):
    K, M, B = 5, 16, 17
    lens = lens_for(B, K)
    model, V, dom, items, off, rel = plain_inputs(D, lens, 5)
    ranked = model.rank_candidates_from_vectors(V, dom, (items, off), k=K)
    for metric in ("dot", "cosine"):
        one = model.diversify((items, off), rel, k=K, lam=1.0, metric=metric, shortlist=M)
        assert torch.equal(one.ids, ranked.ids) and torch.equal(one.positions, ranked.positions) and bits(one.scores) == bits(ranked.scores)
        assert bits(one.values[one.ids >= 0]) == bits(ranked.scores[ranked.ids >= 0])       # (lam = 1: v = 1 * rel - 0 * m)
        res = model.diversify((items, off), rel, k=K, lam=0.3, metric=metric, shortlist=M)
        assert torch.equal(res.ids[:, 0], ranked.ids[:, 0]) and bits(res.scores[:, 0]) == bits(ranked.scores[:, 0])   # pick 1: neither lam nor metric
        assert bool((res.max_sims[:, 0][res.ids[:, 0] >= 0] == 0).all())
        rows = [b for b in range(B) if int(res.ids[b, 1]) >= 0]
        assert len(rows) >= 8
        for b in rows:
            _, sc = model.neighbors(res.ids[b, 1:2], k=1, metric=metric, pool=res.ids[b, 0:1], exclude_self=False)
            assert bits(sc[0, 0]) == bits(res.max_sims[b, 1]), (D, metric, b)


def test_a_row_alone_is_the_row_in_a_batch_and_chunks_change_nothing(monkeypatch):
    from amid_amd import model_seq
    D, K, M, B = 64, 5, 16, 17
    lens = lens_for(B, K)
    model, V, dom, items, off, rel = plain_inputs(D, lens, 6)
    want = model.diversify((items, off), rel, k=K, lam=0.7, metric="cosine", shortlist=M)
    for b in range(B):
        o0, o1 = int(off[b]), int(off[b + 1])
        alone = model.diversify((items[o0:o1], torch.tensor([0, o1 - o0])), rel[o0:o1], k=K, lam=0.7, metric="cosine", shortlist=M)
        for x, y in zip(alone, want):
            assert bits(x[0]) == bits(y[b]), b
    monkeypatch.setattr(model_seq.SASRec, "DIVERSIFY_ROWS", 2)
    monkeypatch.setattr(model_seq.SASRec, "DIVERSIFY_CANDS", 64)
    got = model.diversify((items, off), rel, k=K, lam=0.7, metric="cosine", shortlist=M)
    for x, y in zip(got, want):
        assert x.dtype == y.dtype and x.shape == y.shape and bits(x) == bits(y)
    # a [B, C] tensor with a [B, C] relevance is the same lists as the pair
    rect = torch.stack([torch.randperm(N_ITEMS)[:40] for _ in range(3)])
    r = model.rank_candidates_from_vectors(V[:3], dom[:3], rect, k=None, list_scores=True).list_scores
    a = model.diversify(rect, r.reshape(3, 40), k=K, shortlist=M)
    b_ = model.diversify((rect.reshape(-1), torch.arange(4) * 40), r, k=K, lam=0.7, metric="cosine", shortlist=M)
    for x, y in zip(a, b_):
        assert bits(x) == bits(y)
    assert type(a).__name__ == "DiverseLists" and a._fields == ("ids", "scores", "values", "max_sims", "positions") and a.ids.is_cuda


@pytest.mark.parametrize("kind", ("sasrec", "gru4rec", "bert4rec"))
def test_recommend_diverse_is_recommend_then_diversify(kind):
    D = 64 if kind == "sasrec" else 128
    model = model_of(D, kind)
    g = torch.Generator().manual_seed(2)
    B, T = 8, 20
    s1, s2 = torch.randint(1, N_ITEMS - 1, (B, T), generator=g), torch.randint(1, N_ITEMS - 1, (B, T), generator=g)
    dom = torch.arange(B) % 2
    for K, M, lam, metric, pool, ex in ((5, 16, 0.7, "cosine", None, False), (10, None, 0.3, "dot", None, True),
                                        (5, 16, 0.5, "cosine", torch.arange(3, 15), True)):
        got = model.recommend_diverse(s1, s2, dom, k=K, lam=lam, metric=metric, shortlist=M, pool=pool, exclude_history=ex)
        m = M if M is not None else 100
        ids, sc = model.recommend(s1, s2, dom, k=m, pool=pool, exclude_history=ex)
        if pool is None:
            want = model.diversify(ids, sc, k=K, lam=lam, metric=metric, shortlist=m)
        else:                                                           # 12 candidates for a shortlist of 16: the padding is left out
            assert bool((ids[:, -1] == -1).all())
            n = (ids >= 0).sum(1).cpu()
            off = torch.cat((torch.zeros(1, dtype=torch.int64), torch.cumsum(n, 0)))
            want = model.diversify((ids[ids >= 0], off), sc[ids >= 0], k=K, lam=lam, metric=metric, shortlist=m)
        for x, y in zip(got, want):
            assert x.dtype == y.dtype and bits(x) == bits(y), (kind, K, M)
        assert bool((got.ids[:, 0] == ids[:, 0]).all())


def test_bad_arguments_and_bad_ids():
    D = 64
    model, V, dom, items, off, rel = plain_inputs(D, [40, 0, 5], 7)
    good = (items, off)
    for kw in (dict(k=0), dict(k=257), dict(lam=-0.1), dict(lam=1.5), dict(lam=float("nan")), dict(k=10, shortlist=9), dict(shortlist=257),
               dict(metric="l2")):
        with pytest.raises(ValueError):
            model.diversify(good, rel, **kw)
    for bad in ((items, off[:-1]), (items, torch.tensor([0, 40, 39, 45])), (items, torch.tensor([0, 40, 40, 44])), (items,)):
        with pytest.raises(ValueError):
            model.diversify(bad, rel)
    with pytest.raises(ValueError):
        model.diversify(good, rel[:-1])
    res = model.diversify(good, rel)                                    # shortlist None: min(256, max(k, 100))
    assert res.ids.shape == (3, 10) and bool((res.ids[1] == -1).all()) and bool(torch.isneginf(res.values[1]).all())
    assert bool((res.positions[1] == -1).all()) and int((res.ids[2] >= 0).sum()) == 5
    outside = items.clone()
    outside[3] = N_ITEMS
    with pytest.raises(IndexError):
        model.diversify((outside, off), rel)
    again = model.diversify(good, rel)                                  # (the flag does not outlive its IndexError)
    assert bits(again.ids) == bits(res.ids)


# ---- 4. the command line -------------------------------------------------------------------------------------------------------------------------------
def test_cli_diversify(tmp_path):
    from amid_amd.dataset_seq import DualDomainSeqDataset
    from tests.test_gpu_embeddings import _cli_setup, _train_pools
    recommend, root, common, model = _cli_setup(tmp_path)
    K, N = 5, 40
    plain = recommend.main(common + ["--topk", str(K), "--out", str(tmp_path / "plain.npz")])
    recommend.main(common + ["--topk", str(K), "--out", str(tmp_path / "one.npz"), "--diversify", "1.0"])
    z = np.load(tmp_path / "one.npz")
    assert sorted(z.files) == ["domain_id", "items", "max_sim", "mmr", "scores", "user_id"]
    assert np.array_equal(z["items"], plain["items"]) and z["scores"].tobytes() == plain["scores"].tobytes()
    assert z["mmr"].shape == z["max_sim"].shape == (N, K) and z["mmr"].dtype == z["max_sim"].dtype == np.float32
    assert z["mmr"].tobytes() == z["scores"].tobytes() and (z["max_sim"][:, 0] == 0).all()
    # lambda 0.5 over the top 20: diversify_ranked over recommend_all's top 20
    recommend.main(common + ["--topk", str(K), "--out", str(tmp_path / "half.npz"), "--diversify", "0.5", "--shortlist", "20", "--metric", "dot"])
    ds = DualDomainSeqDataset(seq_len=20, isTrain=False, neg_nums=19, long_length=7, pad_id=447411, seed=1000, csv_path=str(root / "toy_test.csv"))
    sel = recommend.filled_batches(N, 32)
    users = {"seq_d1": torch.from_numpy(ds.seq_d1[sel]).cuda(), "seq_d2": torch.from_numpy(ds.seq_d2[sel]).cuda(),
             "domain_id": torch.from_numpy(ds.domain_id[sel]).cuda()}
    ids, sc = model.recommend_all(users, k=20, pool=tuple(torch.from_numpy(p).cuda() for p in _train_pools(root)))
    want = model.diversify_ranked(ids.reshape(-1, 20)[:N], sc.reshape(-1, 20)[:N], k=K, lam=0.5, metric="dot")
    h = np.load(tmp_path / "half.npz")
    assert np.array_equal(h["items"], want.ids.cpu().numpy()) and h["scores"].tobytes() == bits(want.scores)
    assert h["mmr"].tobytes() == bits(want.values) and h["max_sim"].tobytes() == bits(want.max_sims)
    assert np.array_equal(h["items"][:, 0], plain["items"][:, 0]) and not np.array_equal(h["items"], plain["items"])
    # --candidates: each row's own list (distinct ids), scored by the same path
    rng = np.random.default_rng(5)
    lists = [[] if r % 3 == 0 else rng.choice(np.arange(1, 900), int(rng.integers(1, 30)), replace=False).tolist() for r in range(N)]
    own = np.where(ds.domain_id[:, None] != 0, ds.seq_d2, ds.seq_d1)
    for r in range(1, N, 3):
        lists[r] = list(dict.fromkeys([int(own[r, -1])] + lists[r]))    # an id of the row's history among its candidates
    off = np.concatenate(([0], np.cumsum([len(li) for li in lists]))).astype(np.int64)
    flat = np.array([x for li in lists for x in li], dtype=np.int64)
    np.savez(tmp_path / "cand.npz", offsets=off, items=flat)
    ranked = recommend.main(common + ["--topk", str(K), "--candidates", str(tmp_path / "cand.npz"), "--out", str(tmp_path / "c0.npz")])
    recommend.main(common + ["--topk", str(K), "--candidates", str(tmp_path / "cand.npz"), "--out", str(tmp_path / "c1.npz"), "--diversify", "1.0"])
    c = np.load(tmp_path / "c1.npz")
    assert sorted(c.files) == ["domain_id", "items", "max_sim", "mmr", "positions", "scores", "user_id"]
    assert np.array_equal(c["items"], ranked["items"]) and c["scores"].tobytes() == ranked["scores"].tobytes()
    assert np.array_equal(c["positions"], ranked["positions"])
    recommend.main(common + ["--topk", str(K), "--candidates", str(tmp_path / "cand.npz"), "--out", str(tmp_path / "c2.npz"), "--diversify", "0.5",
                             "--exclude_history", "--list_scores", "--vectors_out", str(tmp_path / "vec.npz")])
    c2 = np.load(tmp_path / "c2.npz")
    assert sorted(c2.files) == ["domain_id", "items", "list_items", "list_scores", "max_sim", "mmr", "offsets", "positions", "scores", "user_id"]
    vec = torch.from_numpy(np.load(tmp_path / "vec.npz")["vectors"]).cuda()
    dom = torch.from_numpy(ds.domain_id)
    scored = model.rank_candidates_from_vectors(vec, dom, (flat, off), k=None, list_scores=True).list_scores
    assert c2["list_scores"].tobytes() == bits(scored)
    rel = scored.clone()
    row = np.repeat(np.arange(N), np.diff(off))
    held = torch.from_numpy(np.array([flat[e] in own[row[e]] for e in range(flat.size)]))
    assert int(held.sum()) >= N // 3 - 1
    rel[held.cuda()] = float("nan")
    want = model.diversify((flat, off), rel, k=K, lam=0.5, metric="cosine", shortlist=100)
    assert np.array_equal(c2["items"], want.ids.cpu().numpy()) and np.array_equal(c2["positions"], want.positions.cpu().numpy())
    assert c2["scores"].tobytes() == bits(want.scores) and c2["mmr"].tobytes() == bits(want.values) and c2["max_sim"].tobytes() == bits(want.max_sims)
    for r in range(N):
        assert not np.isin(c2["items"][r][c2["items"][r] >= 0], own[r]).any(), r
    recommend.main(common + ["--topk", str(K), "--candidates", str(tmp_path / "cand.npz"), "--out", str(tmp_path / "c3.npz"), "--diversify", "0.5",
                             "--exclude_history", "--vectors_in", str(tmp_path / "vec.npz")])
    c3 = np.load(tmp_path / "c3.npz")
    for key in c3.files:
        assert c3[key].tobytes() == c2[key].tobytes(), key
