"""Ranking each row's own candidate list (csrc/rank_lists.hip, SasrecEngine.enqueue_rank_lists, SASRec.rank_candidates /
rank_candidates_from_vectors, recommend.py --candidates), against the forward direction and against float64.

Models with random weights and no training, about 3 000 item rows (long lists hold distinct ids); random finite vectors.  The expectation
of a case is built ONCE from the forward direction: recommend_from_vectors(V, dom, k = len(chunk), pool = chunk) over chunks of at most 256
ids gives S[b, id], the fp32 score of every (row, item) pair.  A list's expected order is the stable sort of its entries by (score
descending, id ascending, position ascending), minus the excluded ids; the new call must return exactly those ids and positions and
bit-equal scores, list_scores must equal S entry for entry, the padding is -1 / -inf / -1.

Shapes: list lengths {0, 1, TILE - 1, TILE, TILE + 1, 700, 2 100} (TILE = 256, the kernel's candidates per tile), B in {1, 8, 9, 40}, k in
{1, 10, 256}, D in {64, 128}, hid in {16, 32, 64}, domains all 0 / all 1 / mixed.  The score launch cuts a row's tiles into units so as to reach
2 048 units, which at these sizes is a unit per tile (the merge launch joins them); every case above one tile runs again with the target
lowered to 1 (one unit walks every tile of a row: the running list and its threshold) and to a third of the tile bound (units of three tiles,
merged).

The independent statement (every case): p = sigmoid(w2 . relu((W1[:, :D] u + b1) + W1[:, D:] E[c]) + b2) from state_dict() in float64 on the
CPU (test_gpu_audience.float64_scores).  Every returned score is within 2e-6 of it (the bar tests/test_gpu_eval.py holds the fused evaluation
to), and every returned entry's float64 score is at least the k-th best float64 score of its list minus 4e-6 (twice that bar: the returned
entry and the entry it displaced may each be off by one bar).  The exact comparison is against fp32 bits, so no case is skipped for
near-ties."""
import numpy as np
import pytest
import torch

from tests.test_gpu_audience import float64_scores

pytestmark = pytest.mark.gpu

TILE = 256                      # RL_TILE of csrc/rank_lists.hip: candidates per tile
LENS = (0, 1, TILE - 1, TILE, TILE + 1, 700, 2100)
BS = (1, 8, 9, 40)
KS = (1, 10, 256)
BAR = 2e-6
N_ITEMS = 3000
_MODELS, _TRUTH = {}, {}


def model_of(kind, D, hid, **kw):
    key = (kind, D, hid, tuple(sorted(kw.items())))
    if key not in _MODELS:
        from amid_amd import model_gru, model_seq
        cls = {"sasrec": model_seq.SASRec, "bert4rec": model_seq.BERT4Rec, "gru4rec": model_gru.GRU4Rec}[kind]
        m = cls(10, D, N_ITEMS, D, 20, hid, 8, False, kw.get("isItC", False), 0.5, 0.3, seed=3)
        m.eval()
        _MODELS[key] = m
    return _MODELS[key]


def vectors(B, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, D, generator=g).cuda().contiguous()


def truth(model, V, tag):
    """(S [B, n_rows] float32 from the forward direction, P64 [B, n_rows] from the float64 formula), once per (model, vectors)."""
    key = (id(model), tag)
    if key not in _TRUTH:
        n_rows, B = model.engine.n_rows, V.shape[0]
        S = np.full((B, n_rows), np.nan, dtype=np.float32)
        dom = torch.zeros(B, dtype=torch.int64).cuda()
        for c0 in range(0, n_rows, 256):
            chunk = torch.arange(c0, min(n_rows, c0 + 256), dtype=torch.int64).cuda()
            ids, sc = model.recommend_from_vectors(V, dom, k=chunk.numel(), pool=chunk)
            ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
            assert (np.sort(ids, axis=1) == chunk.cpu().numpy()[None, :]).all()
            S[np.arange(B)[:, None], ids] = sc
        assert not np.isnan(S).any()
        _TRUTH[key] = (S, float64_scores(model, V, np.arange(n_rows)))
    return _TRUTH[key]


def make_lists(lens, n_rows, seed):
    """Lists of the given lengths: distinct ids 1 .. n_rows - 1 in random order (a list longer than that wraps around)."""
    rng = np.random.default_rng(seed)
    return [np.resize(rng.permutation(np.arange(1, n_rows)), n).astype(np.int64) for n in lens]


def csr(lists):
    off = np.concatenate(([0], np.cumsum([len(li) for li in lists]))).astype(np.int64)
    items = np.concatenate([np.asarray(li, dtype=np.int64) for li in lists]) if off[-1] else np.zeros(0, dtype=np.int64)
    return torch.from_numpy(items), torch.from_numpy(off)


def tile_bound(lists):
    return (sum(len(li) for li in lists) + TILE - 1) // TILE + len(lists)


def call(fn, wgs=0):
    """fn() with the score launch's target unit count set to wgs for the call (0: the default, 2 048 -- at these sizes a unit per tile)."""
    from amid_amd._lib import lib
    lib().value("amid_rank_lists_target_workgroups", wgs)
    try:
        return fn()
    finally:
        lib().value("amid_rank_lists_target_workgroups", 0)


def check(tag, res, lists, S, P64, k, removed=None, want_list_scores=True):
    """Exact against the forward direction, and the float64 statement, for every row."""
    B = len(lists)
    if want_list_scores:
        want = np.concatenate([S[b, lists[b]] for b in range(B)]) if sum(map(len, lists)) else np.zeros(0, np.float32)
        got = res.list_scores.cpu().numpy()
        assert got.dtype == np.float32 and got.shape == want.shape and got.tobytes() == want.tobytes(), tag
    else:
        assert res.list_scores is None
    if k is None:
        assert res.ids is None and res.scores is None and res.positions is None
        return
    assert res.ids.dtype == torch.int64 and res.positions.dtype == torch.int64 and res.scores.dtype == torch.float32
    assert res.ids.shape == res.scores.shape == res.positions.shape == (B, k) and res.ids.is_cuda
    ids, sc, pos = res.ids.cpu().numpy(), res.scores.cpu().numpy(), res.positions.cpu().numpy()
    for b in range(B):
        li = np.asarray(lists[b], dtype=np.int64)
        at = np.arange(len(li))
        if removed is not None and len(li):
            at = at[~np.isin(li, np.asarray(sorted(removed[b]), dtype=np.int64))]
        s = S[b, li[at]]
        o = at[np.lexsort((at, li[at], -s.astype(np.float64)))]
        n = min(k, len(o))
        assert np.array_equal(ids[b][:n], li[o[:n]]) and (ids[b][n:] == -1).all(), (tag, b, ids[b][:8], li[o[:8]])
        assert np.array_equal(pos[b][:n], o[:n]) and (pos[b][n:] == -1).all(), (tag, b, pos[b][:8], o[:8])
        assert sc[b][:n].tobytes() == S[b, li[o[:n]]].tobytes() and np.isneginf(sc[b][n:]).all(), (tag, b)
        if n == 0:
            continue
        p = P64[b, li[o[:n]]]
        err = np.abs(sc[b][:n].astype(np.float64) - p)
        assert (err <= BAR).all(), (tag, b, float(err.max()))
        kth = np.sort(P64[b, li[at]])[::-1][n - 1]
        assert (p >= kth - 2 * BAR).all(), (tag, b, float((kth - p).max()))


def domains(layout, B):
    if layout == "zeros":
        return torch.zeros(B, dtype=torch.int64)
    if layout == "ones":
        return torch.ones(B, dtype=torch.int64)
    return torch.arange(B, dtype=torch.int64) % 2


def cases(n_rows):
    """(name, the lists of the first B rows): every length alone, every B with the lengths rotating through its rows, and the lopsided ones."""
    out = [(f"one list of {n}", make_lists((n,), n_rows, n)) for n in LENS]
    for B in BS[1:]:
        out.append((f"{B} rows", make_lists([LENS[(b + B) % len(LENS)] for b in range(B)], n_rows, B)))
    out.append(("every list empty", make_lists((0,) * 9, n_rows, 1)))
    out.append(("all but one empty", make_lists((0,) * 5 + (700,) + (0,) * 3, n_rows, 2)))
    out.append(("one long among 39 of one entry", make_lists((1,) * 17 + (2100,) + (1,) * 22, n_rows, 3)))
    return out


# ---- exact against the forward direction, and against float64 -----------------------------------------------------------------------------------
@pytest.mark.parametrize("hid", (16, 32, 64))
@pytest.mark.parametrize("D", (64, 128))
def test_ranked_lists_are_the_forward_scores_sorted(D, hid):
    model = model_of("sasrec", D, hid)
    V = vectors(40, D, seed=D + hid)
    S, P64 = truth(model, V, "v40")
    for ci, (name, lists) in enumerate(cases(model.engine.n_rows)):
        B = len(lists)
        items, off = csr(lists)
        many = max(len(li) for li in lists) > TILE
        layouts = ("zeros", "ones", "mixed") if name == "40 rows" else (("zeros", "ones", "mixed")[ci % 3],)
        for layout in layouts:
            dom = domains(layout, B)
            for k in KS:
                for wgs in ((0, 1, max(1, tile_bound(lists) // 3)) if many else (0,)):
                    res = call(lambda: model.rank_candidates_from_vectors(V[:B], dom, (items, off), k=k, list_scores=True), wgs)
                    check((D, hid, name, layout, k, wgs), res, lists, S, P64, k)
    # the top-K alone and the scores alone are the same arrays
    name, lists = cases(model.engine.n_rows)[9]
    items, off = csr(lists)
    B = len(lists)
    res = model.rank_candidates_from_vectors(V[:B], domains("mixed", B), (items.cuda(), off.cuda()), k=10)
    check((D, hid, "top-K alone"), res, lists, S, P64, 10, want_list_scores=False)
    res = model.rank_candidates_from_vectors(V[:B], domains("mixed", B), (items.tolist(), off.numpy()), k=None, list_scores=True)
    check((D, hid, "scores alone"), res, lists, S, P64, None)


def test_rectangular_candidates():
    D, B, C = 64, 8, 300
    model = model_of("sasrec", D, 32)
    V = vectors(40, D, seed=D + 32)
    S, P64 = truth(model, V, "v40")
    rect = np.stack(make_lists((C,) * B, model.engine.n_rows, 11))
    for k in (10, 256):
        for wgs in (0, 1):
            res = call(lambda: model.rank_candidates_from_vectors(V[:B], domains("mixed", B), torch.from_numpy(rect), k=k, list_scores=True), wgs)
            check(("rect", k, wgs), res, list(rect), S, P64, k)
    items, off = csr(list(rect))
    pair = model.rank_candidates_from_vectors(V[:B], domains("mixed", B), (items, off), k=10, list_scores=True)
    for a, b in zip(pair, model.rank_candidates_from_vectors(V[:B], domains("mixed", B), rect, k=10, list_scores=True)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("kind", ("gru4rec", "bert4rec"))
def test_gru4rec_and_bert4rec_inherit_it(kind):
    D = 128
    model = model_of(kind, D, 16)
    V = vectors(9, D, seed=5)
    S, P64 = truth(model, V, "v9")
    lists = make_lists((700, 0, 1, 257, 256, 255, 3, 40, 2100), model.engine.n_rows, 4)
    res = model.rank_candidates_from_vectors(V, domains("mixed", 9), csr(lists), k=10, list_scores=True)
    check((kind,), res, lists, S, P64, 10)


# ---- ties -----------------------------------------------------------------------------------------------------------------------------------------
def test_a_repeated_id_ties_in_position_order():
    D = 64
    model = model_of("sasrec", D, 32)
    V = vectors(40, D, seed=D + 32)
    S, P64 = truth(model, V, "v40")
    lists = make_lists((600, 5, 300), model.engine.n_rows, 7)
    free = np.setdiff1d(np.arange(1, model.engine.n_rows), lists[0])
    same = int(free[np.argmax(S[0, free])])                            # (the best of the 2 400 ids the list does not hold: it is in the top 256)
    lists[0][[3, 290, 599]] = same                                     # the same id in two tiles, three times
    lists[1][:] = 9                                                    # nothing but one id
    lists[2][[0, 299]] = lists[2][150]
    for wgs in (0, 1):
        for k in (2, 256):
            res = call(lambda: model.rank_candidates_from_vectors(V[:3], domains("mixed", 3), csr(lists), k=k, list_scores=True), wgs)
            check(("repeated", wgs, k), res, lists, S, P64, k)
    ids, sc, pos = (x.cpu().numpy() for x in res[:3])
    at = int(np.nonzero(ids[0] == same)[0][0])
    assert ids[0][at:at + 3].tolist() == [same] * 3 and pos[0][at:at + 3].tolist() == [3, 290, 599]
    assert sc[0][at:at + 3].tobytes() == sc[0][at:at + 1].tobytes() * 3
    assert ids[1][:5].tolist() == [9] * 5 and pos[1][:5].tolist() == [0, 1, 2, 3, 4] and (ids[1][5:] == -1).all()


def test_equal_table_rows_tie_to_the_lower_id():
    """Four bit-equal table rows (through load_state_dict), copies of the row vector 0 scores highest, so that they lead its lists."""
    from amid_amd import model_seq
    D = 64
    model = model_seq.SASRec(10, D, N_ITEMS, D, 20, 32, 8, False, False, 0.5, 0.3, seed=6)
    model.eval()
    V = vectors(3, D, seed=1)
    before, _ = truth(model, V, "before")
    best = int(np.argmax(before[0, 1:])) + 1
    tied = sorted({best, 40, 2000, 2500} | ({41} if best in (40, 2000, 2500) else set()))
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    sd["item_emb_layer.emb_item.weight"][tied] = sd["item_emb_layer.emb_item.weight"][best].clone()
    model.load_state_dict(sd)
    S, P64 = truth(model, V, "ties")
    lists = make_lists((600, 2100, 4), model.engine.n_rows, 8)
    for li in lists[:2]:                                               # the four in falling id order, in different tiles
        keep = li[~np.isin(li, tied)]
        li[:] = np.resize(keep, len(li))
        li[[5, 270, 280, 590]] = tied[::-1]
    lists[2][:] = tied[::-1]
    for wgs in (0, 1):
        res = call(lambda: model.rank_candidates_from_vectors(V, domains("mixed", 3), csr(lists), k=256, list_scores=True), wgs)
        check(("equal rows", wgs), res, lists, S, P64, 256)
        ids, sc, pos = (x.cpu().numpy() for x in res[:3])
        assert ids[2][:4].tolist() == tied and pos[2][:4].tolist() == [3, 2, 1, 0] and sc[2][:4].tobytes() == sc[2][:1].tobytes() * 4
        assert ids[0][:4].tolist() == tied and pos[0][:4].tolist() == [590, 280, 270, 5] and sc[0][:4].tobytes() == sc[0][:1].tobytes() * 4


# ---- exclusion --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (10, 256))
def test_history_leaves_exactly_its_ids_out(k):
    D, B, T = 64, 9, 20
    model = model_of("sasrec", D, 32)
    V = vectors(40, D, seed=D + 32)
    S, P64 = truth(model, V, "v40")
    n_rows = model.engine.n_rows
    lists = make_lists((700, 12, 300, 0, 257, 2100, 1, 256, 40), n_rows, 9)
    plain = model.rank_candidates_from_vectors(V[:B], domains("mixed", B), csr(lists), k=k, list_scores=True)
    rng = np.random.default_rng(3)
    hist = np.zeros((B, T), dtype=np.int64)
    hist[0, :5] = plain.ids[0][:5].cpu().numpy()                       # its best five
    hist[0, 5:] = lists[0][300:315]
    hist[1, :12] = lists[1]                                            # a list made only of own ids: all padding
    hist[1, 12:] = lists[1][:8]
    hist[2, :] = np.setdiff1d(np.arange(1, n_rows), lists[2])[:T]      # own ids that are not in the list: nothing changes
    hist[4, :] = rng.choice(lists[4], T)                               # repeated ids, in both tiles
    hist[5, :] = lists[5][::105][:T]
    hist[6, :] = lists[6][0]
    hist[7, :] = lists[7][TILE - T:]
    hist[8, :] = np.concatenate((lists[8][:10], lists[0][:10]))        # ids of another row's list among them
    removed = [set(h.tolist()) for h in hist]
    for wgs in (0, 1):
        res = call(lambda: model.rank_candidates_from_vectors(V[:B], domains("mixed", B), csr(lists), k=k, history=hist, list_scores=True), wgs)
        check(("history", k, wgs), res, lists, S, P64, k, removed=removed)
    assert torch.equal(res.list_scores, plain.list_scores)
    assert (res.ids[1] == -1).all() and torch.isneginf(res.scores[1]).all() and (res.positions[1] == -1).all()
    for b in (2, 3):
        assert torch.equal(res.ids[b], plain.ids[b]) and torch.equal(res.scores[b], plain.scores[b]) and torch.equal(res.positions[b], plain.positions[b])
    assert not np.isin(res.ids[0].cpu().numpy(), hist[0]).any() and (res.ids[6] == -1).all()


# ---- bad ids ----------------------------------------------------------------------------------------------------------------------------------------
def test_ids_outside_the_table_raise_and_score_nan():
    D, B = 64, 3
    model = model_of("sasrec", D, 32)
    eng = model.engine
    V = vectors(40, D, seed=D + 32)
    S, P64 = truth(model, V, "v40")
    lists = make_lists((300, 5, 40), eng.n_rows, 12)
    bad = [li.copy() for li in lists]
    bad[0][7], bad[0][290] = eng.n_rows, -1
    with pytest.raises(IndexError):
        model.rank_candidates_from_vectors(V[:B], domains("mixed", B), csr(bad), k=10)
    with pytest.raises(IndexError):
        model.rank_candidates_from_vectors(V[:B], domains("mixed", B), csr(bad), k=None, list_scores=True)
    # the engine method directly: the output is read before the flag is
    items, off = (t.cuda() for t in csr(bad))
    dom = domains("mixed", B).cuda()
    ls = torch.zeros(items.numel(), device="cuda")
    ids = torch.zeros(B, 10, dtype=torch.int64, device="cuda")
    sc, pos = torch.zeros(B, 10, device="cuda"), torch.zeros(B, 10, dtype=torch.int64, device="cuda")
    flags = eng.flags_holder()
    eng.stream.wait_stream(torch.cuda.current_stream())
    eng.enqueue_rank_lists(V[:B], 0, dom, items, off, items.numel(), None, None, None, None, ls, None, None, None, flags.err)
    eng.enqueue_rank_lists(V[:B], 0, dom, items, off, items.numel(), None, None, None, 10, None, ids, sc, pos, flags.err)
    torch.cuda.current_stream().wait_stream(eng.stream)
    got = ls.cpu().numpy()
    with pytest.raises(IndexError):
        eng.check_index_error(flags)
    want = np.concatenate([S[b, np.clip(bad[b], 0, eng.n_rows - 1)] for b in range(B)])
    where = np.zeros(len(got), dtype=bool)
    where[[7, 290]] = True
    assert np.isnan(got[where]).all() and got[~where].tobytes() == want[~where].tobytes()
    from amid_amd.model_seq import RankedLists
    good = [np.delete(bad[0], [7, 290]), bad[1], bad[2]]               # the bad entries never enter the top-K; the positions are the list's
    res = RankedLists(ids, sc, pos, None)
    shift = lambda p: np.where(p > 290, p - 2, np.where(p > 7, p - 1, p))      # noqa: E731
    pos0 = pos[0].cpu().numpy()
    assert not np.isin(pos0, (7, 290)).any()
    pos[0] = torch.from_numpy(shift(pos0)).cuda()
    check(("bad ids",), res, good, S, P64, 10, want_list_scores=False)
    clean = model.rank_candidates_from_vectors(V[:B], domains("mixed", B), csr(lists), k=10, list_scores=True)      # (the flag does not outlive its IndexError)
    check(("clean",), clean, lists, S, P64, 10)


def test_offsets_outside_the_candidates_are_clamped_and_flagged():
    """The engine method with offsets the model API would refuse: a falling pair is an empty list, an offset past n_cand is clamped, both
    raise the flag, and nothing past cand[n_cand) is read (the entries behind it are ids outside the table)."""
    D, B = 64, 4
    model = model_of("sasrec", D, 32)
    eng = model.engine
    V = vectors(40, D, seed=D + 32)
    S, P64 = truth(model, V, "v40")
    lists = make_lists((300, 5, 40, 7), eng.n_rows, 13)
    items, _ = csr(lists)
    n = items.numel()
    padded = torch.cat((items, torch.full((600,), 2 ** 40, dtype=torch.int64))).cuda()
    off = torch.tensor([0, 300, 295, 345, n + 500], dtype=torch.int64).cuda()      # row 1 falls; row 2 = [295, 345); row 3 = [345, n)
    dom = domains("mixed", B).cuda()
    ids = torch.zeros(B, 256, dtype=torch.int64, device="cuda")
    sc, pos = torch.zeros(B, 256, device="cuda"), torch.zeros(B, 256, dtype=torch.int64, device="cuda")
    ls = torch.full((n,), -5.0, device="cuda")
    flags = eng.flags_holder()
    eng.stream.wait_stream(torch.cuda.current_stream())
    eng.enqueue_rank_lists(V[:B], 0, dom, padded, off, n, None, None, None, 256, ls, ids, sc, pos, flags.err)
    torch.cuda.current_stream().wait_stream(eng.stream)
    torch.cuda.synchronize()
    with pytest.raises(IndexError):
        eng.check_index_error(flags)
    flat = items.numpy()
    seen = [flat[:300], flat[:0], flat[295:345], flat[345:n]]
    from amid_amd.model_seq import RankedLists
    check(("clamped",), RankedLists(ids, sc, pos, None), seen, S, P64, 256, want_list_scores=False)
    got = ls.cpu().numpy()
    assert got[:295].tobytes() == S[0, flat[:295]].tobytes() and got[345:].tobytes() == S[3, flat[345:]].tobytes()
    assert got[300:345].tobytes() == S[2, flat[300:345]].tobytes()                 # (entries 295 .. 299 belong to two rows: either's score)


def test_overlapping_lists_stay_inside_the_workspace():
    """Offsets 0, n, 0, n, ..: twenty rows that each name the whole array (and twenty falling pairs), 2 000 tiles where the workspace was
    sized for ceil(n / 256) + B = 140.  The prefix is cut there and the flag raised: row 0 (the first 100 units) is exact, the rows behind
    the cut are padding, every score written is the score of a row that names the entry, and nothing outside the workspace is written (the
    tensors allocated around it keep their values)."""
    D, B, n = 64, 40, 25600
    model = model_of("sasrec", D, 32)
    eng = model.engine
    V = vectors(40, D, seed=D + 32)
    S, P64 = truth(model, V, "v40")
    flat = make_lists((n,), eng.n_rows, 14)[0]
    items = torch.from_numpy(flat).cuda()
    off = torch.tensor([0 if b % 2 == 0 else n for b in range(B + 1)], dtype=torch.int64).cuda()
    dom = domains("mixed", B).cuda()
    flags = eng.flags_holder()
    eng.stream.wait_stream(torch.cuda.current_stream())
    eng._rank_lists_workspace(B, n, 10)                                # (the workspace exists before its neighbours are allocated)
    with torch.cuda.stream(eng.stream):
        guard = [torch.full((1 << 20,), 7, dtype=torch.int32, device="cuda") for _ in range(4)]
        ids = torch.zeros(B, 10, dtype=torch.int64, device="cuda")
        sc, pos = torch.zeros(B, 10, device="cuda"), torch.zeros(B, 10, dtype=torch.int64, device="cuda")
        ls = torch.full((n,), -5.0, device="cuda")
    eng.enqueue_rank_lists(V[:B], 0, dom, items, off, n, None, None, None, 10, ls, ids, sc, pos, flags.err)
    torch.cuda.current_stream().wait_stream(eng.stream)
    torch.cuda.synchronize()
    with pytest.raises(IndexError):
        eng.check_index_error(flags)
    assert all(bool((g == 7).all()) for g in guard)
    from amid_amd.model_seq import RankedLists
    check(("overlap",), RankedLists(ids[:1], sc[:1], pos[:1], None), [flat], S, P64, 10, want_list_scores=False)
    assert (ids[3:] == -1).all() and torch.isneginf(sc[3:]).all() and (pos[3:] == -1).all() and (ids[1] == -1).all()
    got = ls.cpu().numpy()
    assert ((got == S[0, flat]) | (got == S[2, flat])).all()


# ---- identity with the existing paths ---------------------------------------------------------------------------------------------------------------
def _eval_batch(n_rows, B=8, T=20, neg=31, seed=2):
    g = torch.Generator().manual_seed(seed)
    s1 = torch.randint(1, n_rows - 1, (B, T), generator=g)
    s2 = torch.randint(1, n_rows - 1, (B, T), generator=g)
    s1[:, :5], s2[1::2, :9] = n_rows - 1, n_rows - 1                  # some padding in front
    dom = torch.arange(B) % 2
    return {"seq_d1": s1.cuda(), "seq_d2": s2.cuda(), "domain_id": dom.cuda(), "i_node": torch.randint(1, n_rows - 1, (B,), generator=g).cuda(),
            "neg_samples": torch.randint(1, n_rows - 1, (B, neg), generator=g).cuda()}


@pytest.mark.parametrize("kind", ("sasrec", "itc", "bert4rec", "gru4rec"))
def test_list_scores_are_the_evaluation_forward_s(kind):
    D = 64 if kind in ("sasrec", "itc") else 128
    model = model_of("sasrec" if kind == "itc" else kind, D, 16, **({"isItC": True} if kind == "itc" else {}))
    b = _eval_batch(model.engine.n_rows)
    B = 8
    with torch.no_grad():
        outs = model(None, b["i_node"], b["neg_samples"], b["seq_d1"], b["seq_d2"], None, None, False)
    want = torch.where(b["domain_id"][:, None] != 0, outs[1].reshape(B, -1), outs[0].reshape(B, -1))
    cand = torch.cat((b["i_node"][:, None], b["neg_samples"]), dim=1)
    res = model.rank_candidates(b["seq_d1"], b["seq_d2"], b["domain_id"], cand, k=None, list_scores=True)
    assert res.ids is None and res.list_scores.shape == (B * 32,)
    assert res.list_scores.reshape(B, 32).cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    # ... and rank_candidates is encode_users followed by rank_candidates_from_vectors, exclusion included
    users = {"seq_d1": b["seq_d1"][None], "seq_d2": b["seq_d2"][None], "domain_id": b["domain_id"][None]}
    vec = model.encode_users(users)[0]
    own = torch.where(b["domain_id"][:, None] != 0, b["seq_d2"], b["seq_d1"])
    lists = make_lists((40, 0, 300, 7, 1, 257, 20, 700), model.engine.n_rows, 5)
    for b_, li in enumerate(lists):
        if len(li) >= 7:
            li[:6] = own[b_, -6:].cpu().numpy()                        # ids of the history among the candidates
    for ex in (False, True):
        one = model.rank_candidates(b["seq_d1"], b["seq_d2"], b["domain_id"], csr(lists), k=10, exclude_history=ex, list_scores=True)
        two = model.rank_candidates_from_vectors(vec, b["domain_id"], csr(lists), k=10, history=own if ex else None, list_scores=True)
        for x, y in zip(one, two):
            assert x.dtype == y.dtype and x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), (kind, ex)
        same_row = np.array([[int(i) in set(own[r].tolist()) for i in row] for r, row in enumerate(one.ids.cpu().numpy())])
        assert (not same_row.any()) if ex else same_row.any(), (kind, ex)      # (row 3 returns its whole list, six own ids in it)


def test_every_list_the_pool_is_recommend_from_vectors():
    D, B = 128, 9
    model = model_of("sasrec", D, 32)
    V = vectors(B, D, seed=3)
    rng = np.random.default_rng(1)
    pool = np.sort(rng.choice(np.arange(1, model.engine.n_rows), 150, replace=False)).astype(np.int64)
    hist = torch.from_numpy(rng.choice(pool, (B, 20)))
    dom = domains("mixed", B)
    for k in (10, 256):                                                # 256 > the pool: the padding too
        for h in (None, hist):
            want_i, want_s = model.recommend_from_vectors(V, dom, k=k, pool=torch.from_numpy(pool), history=h)
            res = model.rank_candidates_from_vectors(V, dom, torch.from_numpy(np.tile(pool, (B, 1))), k=k, history=h)
            assert torch.equal(res.ids, want_i) and res.scores.cpu().numpy().tobytes() == want_s.cpu().numpy().tobytes()
            some = (res.ids >= 0).cpu().numpy()
            assert some[:, :10].all() and (pool[res.positions.cpu().numpy()[some]] == res.ids.cpu().numpy()[some]).all()


# ---- chunking and the argument checks -------------------------------------------------------------------------------------------------------------
def test_the_rows_go_in_chunks(monkeypatch):
    from amid_amd import model_seq
    D, B = 64, 40
    model = model_of("sasrec", D, 32)
    V = vectors(40, D, seed=D + 32)
    lists = cases(model.engine.n_rows)[9][1]
    hist = np.stack([np.resize(li[:20], 20) if len(li) else np.zeros(20, np.int64) for li in lists])
    want = model.rank_candidates_from_vectors(V, domains("mixed", B), csr(lists), k=10, history=hist, list_scores=True)
    for rows, cands in ((3, 1 << 26), (65536, 500), (7, 300)):
        monkeypatch.setattr(model_seq.SASRec, "RANK_LISTS_ROWS", rows)
        monkeypatch.setattr(model_seq.SASRec, "RANK_LISTS_CANDS", cands)
        got = model.rank_candidates_from_vectors(V, domains("mixed", B), csr(lists), k=10, history=hist, list_scores=True)
        for x, y in zip(got, want):
            assert torch.equal(x, y) or x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), (rows, cands)


def test_a_chunk_of_empty_lists_with_scores_only(monkeypatch):
    from amid_amd import model_seq
    D = 64
    model = model_of("sasrec", D, 32)
    V = vectors(40, D, seed=D + 32)
    S, P64 = truth(model, V, "v40")
    lists = make_lists((0, 0, 0, 5, 0, 0, 0, 0, 300, 0, 0, 0), model.engine.n_rows, 15)
    monkeypatch.setattr(model_seq.SASRec, "RANK_LISTS_ROWS", 3)
    for k in (None, 10):
        res = model.rank_candidates_from_vectors(V[:12], domains("mixed", 12), csr(lists), k=k, list_scores=True)
        check(("empty chunks", k), res, lists, S, P64, k)
    res = model.rank_candidates_from_vectors(V[:3], domains("mixed", 3), csr(lists[:3]), k=None, list_scores=True)
    assert res.ids is None and res.list_scores.shape == (0,)


def test_bad_arguments_raise_value_error():
    D, B = 64, 4
    model = model_of("sasrec", D, 32)
    V, dom = vectors(B, D, seed=1), domains("mixed", B)
    good = (torch.arange(1, 9), torch.tensor([0, 2, 2, 5, 8]))
    for k in (0, 257, -1):
        with pytest.raises(ValueError):
            model.rank_candidates_from_vectors(V, dom, good, k=k)
    with pytest.raises(ValueError):
        model.rank_candidates_from_vectors(V, dom, good, k=None)      # nothing asked for
    for bad in ((torch.arange(1, 9), torch.tensor([0, 2, 5, 8])), (torch.arange(1, 9), torch.tensor([1, 2, 2, 5, 8])),
                (torch.arange(1, 9), torch.tensor([0, 2, 1, 5, 8])), (torch.arange(1, 9), torch.tensor([0, 2, 2, 5, 9])),
                (torch.arange(1, 9), torch.tensor([0, 2, 2, 5, 7])), torch.arange(1, 9), torch.ones(3, 5, dtype=torch.int64), (torch.arange(3),)):
        with pytest.raises(ValueError):
            model.rank_candidates_from_vectors(V, dom, bad, k=3)
    with pytest.raises(ValueError):
        model.rank_candidates_from_vectors(V[:, :32], dom, good, k=3)
    with pytest.raises(ValueError):
        model.rank_candidates_from_vectors(V, dom, good, k=3, history=torch.ones(3, 5, dtype=torch.int64))
    itc = model_of("sasrec", 64, 16, isItC=True)                       # a comp model encodes exactly bs rows
    b = _eval_batch(itc.engine.n_rows)
    with pytest.raises(ValueError):
        itc.rank_candidates(b["seq_d1"][:5], b["seq_d2"][:5], b["domain_id"][:5], torch.ones(5, 3, dtype=torch.int64), k=2)


# ---- the command line -------------------------------------------------------------------------------------------------------------------------------
def test_cli_candidates(tmp_path):
    from amid_amd.dataset_seq import DualDomainSeqDataset
    from tests.test_gpu_embeddings import _cli_setup
    recommend, root, common, model = _cli_setup(tmp_path)
    K, N = 5, 40
    ds = DualDomainSeqDataset(seq_len=20, isTrain=False, neg_nums=19, long_length=7, pad_id=447411, seed=1000, csv_path=str(root / "toy_test.csv"))
    own = np.where(ds.domain_id[:, None] != 0, ds.seq_d2, ds.seq_d1)
    rng = np.random.default_rng(5)
    lists = []
    for r in range(N):                                                 # up to 30 ids of both domains' ranges, the held-out item and two of the row's history among them
        li = rng.integers(1, 900, int(rng.integers(0, 30))).tolist()
        if r % 3 == 0:
            li = []
        elif len(li) >= 4:
            li[0], li[1], li[3] = int(ds.i_node[r]), int(own[r, -1]), int(own[r, -1])
        lists.append(li)
    off = np.concatenate(([0], np.cumsum([len(li) for li in lists]))).astype(np.int64)
    flat = np.array([x for li in lists for x in li], dtype=np.int64)
    np.savez(tmp_path / "cand.npz", offsets=off, items=flat, user_id=ds.user_nodes)
    (tmp_path / "cand.txt").write_text("".join(" ".join(str(x) for x in li) + "\n" for li in lists))
    out = recommend.main(common + ["--topk", str(K), "--candidates", str(tmp_path / "cand.npz"), "--out", str(tmp_path / "a.npz"),
                                   "--vectors_out", str(tmp_path / "vec.npz")])
    z = np.load(tmp_path / "a.npz")
    assert sorted(z.files) == ["domain_id", "items", "positions", "scores", "user_id"]
    sel = recommend.filled_batches(N, 32)
    users = {"seq_d1": torch.from_numpy(ds.seq_d1[sel]).cuda(), "seq_d2": torch.from_numpy(ds.seq_d2[sel]).cuda(),
             "domain_id": torch.from_numpy(ds.domain_id[sel]).cuda()}
    vec = model.encode_users(users).reshape(-1, 64)[:N].contiguous()
    dom = torch.from_numpy(ds.domain_id)
    want = model.rank_candidates_from_vectors(vec, dom, (flat, off), k=K, list_scores=True)
    assert np.array_equal(z["user_id"], ds.user_nodes) and np.array_equal(z["domain_id"], ds.domain_id)
    assert np.array_equal(z["items"], want.ids.cpu().numpy()) and np.array_equal(z["positions"], want.positions.cpu().numpy())
    assert z["scores"].dtype == np.float32 and z["scores"].tobytes() == want.scores.cpu().numpy().tobytes()
    assert np.array_equal(out["items"], z["items"]) and (z["items"][::3] == -1).all() and (z["items"] >= 0).any()
    # the text form of the same lists, and --vectors_in on the file --vectors_out wrote: the same file
    recommend.main(common + ["--topk", str(K), "--candidates", str(tmp_path / "cand.txt"), "--out", str(tmp_path / "b.npz")])
    recommend.main(common + ["--topk", str(K), "--candidates", str(tmp_path / "cand.npz"), "--out", str(tmp_path / "c.npz"),
                             "--vectors_in", str(tmp_path / "vec.npz")])
    for name in ("b.npz", "c.npz"):
        z2 = np.load(tmp_path / name)
        assert sorted(z2.files) == sorted(z.files)
        for key in z.files:
            assert z[key].dtype == z2[key].dtype and z[key].shape == z2[key].shape and z[key].tobytes() == z2[key].tobytes(), (name, key)
    # --exclude_history removes the held ids; --list_scores adds the three arrays
    recommend.main(common + ["--topk", str(K), "--candidates", str(tmp_path / "cand.npz"), "--out", str(tmp_path / "d.npz"), "--exclude_history",
                             "--list_scores"])
    z3 = np.load(tmp_path / "d.npz")
    assert sorted(z3.files) == ["domain_id", "items", "list_items", "list_scores", "offsets", "positions", "scores", "user_id"]
    held = model.rank_candidates_from_vectors(vec, dom, (flat, off), k=K, history=own, list_scores=True)
    assert np.array_equal(z3["items"], held.ids.cpu().numpy()) and np.array_equal(z3["positions"], held.positions.cpu().numpy())
    assert z3["scores"].tobytes() == held.scores.cpu().numpy().tobytes()
    assert np.array_equal(z3["offsets"], off) and np.array_equal(z3["list_items"], flat)
    assert z3["list_scores"].tobytes() == want.list_scores.cpu().numpy().tobytes()
    n_gone = 0
    for r in range(N):
        assert not np.isin(z3["items"][r][z3["items"][r] >= 0], own[r]).any(), r
        n_gone += int(np.isin(z["items"][r][z["items"][r] >= 0], own[r]).sum())
    assert n_gone > 0
    # --history full: the held-out item leaves too
    recommend.main(common + ["--topk", "30", "--candidates", str(tmp_path / "cand.npz"), "--out", str(tmp_path / "e.npz"), "--exclude_history",
                             "--history", "full"])
    z4 = np.load(tmp_path / "e.npz")
    for r in range(N):
        assert int(ds.i_node[r]) not in z4["items"][r].tolist() and not np.isin(z4["items"][r][z4["items"][r] >= 0], own[r, 1:]).any(), r
    # what is refused
    (tmp_path / "short.txt").write_text("".join(" ".join(str(x) for x in li) + "\n" for li in lists[:-1]))
    with pytest.raises(SystemExit) as e:
        recommend.main(common + ["--candidates", str(tmp_path / "short.txt"), "--out", str(tmp_path / "no.npz")])
    assert "39" in str(e.value) and "40" in str(e.value)
    np.savez(tmp_path / "other.npz", offsets=off, items=flat, user_id=ds.user_nodes[::-1].copy())
    with pytest.raises(SystemExit) as e:
        recommend.main(common + ["--candidates", str(tmp_path / "other.npz"), "--out", str(tmp_path / "no.npz")])
    assert "user_id" in str(e.value)
    for extra in (["--audience_of", "all"], ["--similar_items", "all"]):
        with pytest.raises(SystemExit):
            recommend.main(common + ["--candidates", str(tmp_path / "cand.npz"), "--out", str(tmp_path / "no.npz")] + extra)
    for alone in (["--exclude_history"], ["--list_scores"]):
        with pytest.raises(SystemExit):
            recommend.main(common + ["--out", str(tmp_path / "no.npz")] + alone)
    with pytest.raises(SystemExit):                                    # a joint job is refused, as for the other modes
        recommend.main([a if a != "toy" else "toy+toy" for a in common] + ["--candidates", str(tmp_path / "cand.npz")])
    assert not (tmp_path / "no.npz").exists()
