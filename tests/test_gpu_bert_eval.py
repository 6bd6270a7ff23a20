"""BERT4Rec's fused evaluation batch (Bert4recEngine._enqueue_eval_encoders + SasrecEngine.enqueue_eval: test(), train_sr.py:31-128) in both
of its forms -- the encoder as ONE launch (csrc/bert_seq_infer.hip) and the strips staged over the live list with nothing saved -- against
the launches it replaces (enqueue_forward over both domains + amid_positive_rank_f32), bit for bit, against the oracle, and through
train_sr.test(), full_ranks() and recommend()."""
import json

import numpy as np
import pytest
import torch

from oracle import amid_oracle as orc

pytestmark = pytest.mark.gpu
FIX = 1e-7
D = orc.BERT_HIDDEN
N_ITEMS, HID = 3000, 32
KEYS = ("i_node", "neg_samples", "seq_d1", "seq_d2", "label", "domain_id")


def make_engine(P, T, **kw):
    from amid_amd.engine_bert import Bert4recEngine
    n_rows = P["item_emb_layer.emb_item.weight"].shape[0]
    hid = P["predictModule.fc.0.weight"].shape[0]
    eng = Bert4recEngine(n_rows, D, T, hid, lr=5e-4, seed=0, **kw)
    eng.load_state_dict(P)
    return eng


def eval_batch(B, T, NI, seed, dom=None, n_items=N_ITEMS):
    """As batch_with_masked_keys (tests/test_gpu_bert4rec.py): zeros in seq_d2 (masked keys, model_seq.py:288), row 0 entirely zero (every key
    masked: the -1e9 fill makes the softmax uniform), row 1 without any; labels one-hot on column 0; the positive's own id among the negatives
    of every second row when NI > 4 (an exact tie); dom = 0 / 1: every row of that domain (the live list has an empty half)."""
    b = orc.synthetic_batch(B, T, n_items - 1, pad_id=0, neg=NI - 1, seed=seed)
    g = torch.Generator().manual_seed(seed)
    z = torch.rand(B, T, generator=g) < 0.3
    b["seq_d2"] = torch.where(z, torch.zeros_like(b["seq_d2"]), b["seq_d2"].clamp(min=1))
    b["seq_d2"][0] = 0
    if B > 1:
        b["seq_d2"][1] = b["seq_d2"][1].clamp(min=1)
    b["neg_samples"] = b["neg_samples"].reshape(B, NI - 1)
    if NI > 4:
        b["neg_samples"][::2, 3] = b["i_node"].reshape(B)[::2]
    b["label"] = torch.zeros(B, NI)
    b["label"][:, 0] = 1.0
    if dom is not None:
        b["domain_id"] = torch.full_like(b["domain_id"], dom)
    return b


def old_path(eng, pl, cu):
    """What test() ran for BERT4Rec before: the eval forward over every sequence of both domains with the candidates gathered by K1, then the
    rank kernel."""
    from amid_amd.utils import device_positive_ranks
    eng.load_batch(pl, *(cu[k] for k in KEYS))
    eng.enqueue_prepare(pl, sparse=False)
    eng.enqueue_forward(pl, train=False, with_loss=False)
    eng.sync()
    torch.cuda.current_stream().wait_stream(eng.stream)
    p1, p2 = pl.p1.clone().reshape(pl.shape.B, -1), pl.p2.clone().reshape(pl.shape.B, -1)
    r = device_positive_ranks(p1, p2, cu["domain_id"], FIX)
    r0 = device_positive_ranks(p1, p2, cu["domain_id"], 0.0)
    torch.cuda.synchronize()
    own = torch.where(cu["domain_id"][:, None] != 0, p2, p1)
    return own, r, r0


def poison(eng, pl):
    """NaN into everything an evaluation batch's encoders write or hand on (the forward over both domains has just left the EXPECTED bits in these
    buffers): a launch that skipped a row, a tail strip, a workgroup or an empty live half would otherwise be covered by the stale rows."""
    eng.sync()
    for t in [pl.xg, pl.u] + list(pl.x) + list(pl.q) + list(pl.k) + list(pl.v) + list(pl.o):
        t.fill_(float("nan"))
    if hasattr(pl, "ev_out"):
        pl.ev_out.fill_(-1)
        pl.ev_p.fill_(float("nan"))
        pl.ev_u.fill_(float("nan"))
    torch.cuda.synchronize()


def run_eval(eng, pl, cu, one_launch):
    eng.EVAL_ONE_LAUNCH = one_launch
    poison(eng, pl)
    eng.load_batch(pl, *(cu[k] for k in KEYS))
    eng.enqueue_eval(pl, FIX, with_loss=True, want_scores=True)
    eng.sync()
    eng.check_index_error(pl)
    torch.cuda.current_stream().wait_stream(eng.stream)
    return pl.ev_p.clone(), pl.ev_rank.clone(), pl.ev_rank_raw.clone(), pl.ev_loss_part.clone(), pl.x[2].clone()


def live_rows(x2, cu, B, T):
    """The own-domain sequences' rows of pl.x[2] [2, B, T, D]."""
    x = x2.reshape(2, B, T, D)
    return torch.where(cu["domain_id"][:, None, None] != 0, x[1], x[0])


def check_against_old(eng, pl, cu, B, T, NI, one_launch):
    """One form of the evaluation batch against the launches it replaces, its buffers poisoned in between (run_eval); the one-launch form also
    against the staged form's live rows."""
    own, r, r0 = old_path(eng, pl, cu)
    Tenc = pl.shape.Tenc
    x_old = live_rows(pl.x[2].clone(), cu, B, Tenc)
    p, rk, rk0, lp, x2 = run_eval(eng, pl, cu, one_launch)
    assert bool(torch.isfinite(x_old).all()) and torch.equal(live_rows(x2, cu, B, Tenc), x_old)      # every live row written, with the forward's bits
    assert torch.equal(p, own), (one_launch, float((p - own).abs().max()))
    assert torch.equal(rk, r) and torch.equal(rk0, r0), one_launch
    y = cu["label"]
    want = torch.nn.functional.binary_cross_entropy(own.double(), y.double(), reduction="none").sum(1) / (B * NI)      # train_sr.py:63-64
    assert float((lp.double() - want).abs().max()) <= 1e-6 * float(want.abs().max()) + 1e-9, one_launch
    ties = (own[:, 1:] == own[:, :1]).sum(1).int()
    assert bool((rk - rk0 >= ties).all()), one_launch
    if one_launch:
        xs = live_rows(run_eval(eng, pl, cu, False)[4], cu, B, Tenc)
        assert torch.equal(live_rows(x2, cu, B, Tenc), xs)


def record_launches(monkeypatch, fn):
    from amid_amd._lib import lib
    L = lib()
    names = []
    orig = L.call

    def call(name, *args):
        names.append(name)
        return orig(name, *args)

    monkeypatch.setattr(L, "call", call)
    try:
        fn()
    finally:
        monkeypatch.undo()
    return names


FORMS = [pytest.param(True, id="one_launch"), pytest.param(False, id="staged")]


# ---------------------------------------------------------------------------- the plain model
@pytest.mark.parametrize("one_launch", FORMS)
@pytest.mark.parametrize("B,T,NI", [(1, 1, 2), (3, 16, 5), (7, 17, 5), (9, 33, 130), (16, 50, 100), (5, 64, 1000), (256, 50, 200)])
def test_both_forms_are_bit_identical_to_the_forward_and_rank_kernels(B, T, NI, one_launch):
    """Either form of the evaluation batch gives the bits of enqueue_forward(train=False) + the rank kernel: x[2]'s live rows, the scores, both
    ranks; the loss to 1e-6.  (The one-launch kernel keeps the chains' multiplications by the runtime dropout scale for exactly this: without
    them the compiler fuses other multiply-adds and the rows differ by ~2^-19.)"""
    P = orc.random_params(orc.bert4rec_param_shapes(N_ITEMS, HID), seed=3 + T)
    eng = make_engine(P, T)
    pl = eng.plan(B, T, NI, need_grad=False)
    eng.EVAL_ONE_LAUNCH = True
    assert eng.eval_fused_ok(pl) and eng._eval_one_launch(pl)
    for seed, dom in ((40, None), (41, 0), (42, 1)):
        cu = {k: v.cuda() for k, v in eval_batch(B, T, NI, seed, dom).items()}
        torch.cuda.synchronize()          # (the engine's stream does not wait for torch's)
        check_against_old(eng, pl, cu, B, T, NI, one_launch)


@pytest.mark.parametrize("B,T,NI", [(7, 17, 5), (16, 50, 100)])
def test_staged_form_on_the_fp32_strip_entry_points(B, T, NI, monkeypatch):
    """STRIP_P3 off: the strips multiply with fp32 matrix instructions (amid_bert_strip_*_f32, no tile images); the one-launch kernel does not
    apply, and the staged form hands THOSE entry points the null saved-tensor pointers -- the same bits as the forward, again."""
    P = orc.random_params(orc.bert4rec_param_shapes(N_ITEMS, HID), seed=3 + T)
    eng = make_engine(P, T)
    eng.STRIP_P3 = False
    eng.EVAL_ONE_LAUNCH = True
    pl = eng.plan(B, T, NI, need_grad=False)
    assert eng.eval_fused_ok(pl) and not eng._eval_one_launch(pl)
    for seed, dom in ((40, None), (42, 1)):
        cu = {k: v.cuda() for k, v in eval_batch(B, T, NI, seed, dom).items()}
        torch.cuda.synchronize()
        check_against_old(eng, pl, cu, B, T, NI, False)
    eng.load_batch(pl, *(cu[k] for k in KEYS))
    names = record_launches(monkeypatch, lambda: eng.enqueue_eval(pl, FIX))
    eng.sync()
    assert "amid_bert_strip_qkv_fwd_pro_f32" in names and names.count("amid_bert_strip_oproj_ffn_fwd_f32") == 2
    assert "amid_bert_weight_images_f32" not in names and "amid_bert_seq_fwd_gather_infer_f32" not in names


@pytest.mark.parametrize("one_launch", FORMS)
def test_scores_against_the_oracle(one_launch):
    """The bar test_forward_logits_vs_oracle (tests/test_gpu_bert4rec.py) holds this model's logits to: relmax < 1e-4 on the own-domain scores."""
    from tests.test_gpu_sasrec import relmax
    B, T, NI = 9, 50, 130
    P = orc.random_params(orc.bert4rec_param_shapes(N_ITEMS, HID), seed=11)
    eng = make_engine(P, T)
    pl = eng.plan(B, T, NI, need_grad=False)
    b = eval_batch(B, T, NI, 7)
    with torch.no_grad():
        p1, p2 = orc.bert4rec_forward(P, b["i_node"], b["neg_samples"], b["seq_d1"], b["seq_d2"], None)
    want = torch.where(b["domain_id"][:, None] != 0, p2.reshape(B, -1), p1.reshape(B, -1))
    cu = {k: v.cuda() for k, v in b.items()}
    torch.cuda.synchronize()
    p = run_eval(eng, pl, cu, one_launch)[0]
    e = relmax(p, want)
    print(f"bert eval one_launch={one_launch}: own-domain scores relmax {e:.3e}")
    assert e < 1e-4, (one_launch, e)


def test_launch_counts(monkeypatch):
    B, T, NI = 16, 50, 100
    P = orc.random_params(orc.bert4rec_param_shapes(N_ITEMS, HID), seed=5)
    eng = make_engine(P, T)
    pl = eng.plan(B, T, NI, need_grad=False)
    cu = {k: v.cuda() for k, v in eval_batch(B, T, NI, 3).items()}
    torch.cuda.synchronize()
    eng.load_batch(pl, *(cu[k] for k in KEYS))
    eng.enqueue_eval(pl, FIX)             # (builds the images)
    eng.sync()
    eng.EVAL_ONE_LAUNCH = True
    one = record_launches(monkeypatch, lambda: eng.enqueue_eval(pl, FIX, build_images=False))
    assert one == ["amid_pack_indices_live", "amid_bert_seq_fwd_gather_infer_f32", "amid_eval_head_f32"], one
    built = record_launches(monkeypatch, lambda: eng.enqueue_eval(pl, FIX, build_images=True))
    assert built == ["amid_pack_indices_live", "amid_bert_weight_images_f32", "amid_bert_seq_fwd_gather_infer_f32", "amid_eval_head_f32"], built
    eng.EVAL_ONE_LAUNCH = False
    staged = record_launches(monkeypatch, lambda: eng.enqueue_eval(pl, FIX, build_images=False))
    eng.sync()
    eng.EVAL_ONE_LAUNCH = True
    assert staged == ["amid_pack_indices_live", "amid_embed_fwd_live_f32", "amid_bert_strip_qkv_fwd_pro_p3_f32", "amid_attn_bert_fwd_live_f32",
                      "amid_bert_strip_oproj_ffn_fwd_p3_f32", "amid_attn_bert_fwd_live_f32", "amid_bert_strip_oproj_ffn_fwd_p3_f32",
                      "amid_eval_head_f32"], staged
    for names in (one, built, staged):
        assert "amid_head_fwd_f32" not in names and "amid_positive_rank_f32" not in names


@pytest.mark.parametrize("one_launch", FORMS)
def test_eval_epoch_graph_equals_eager_and_the_old_path_at_the_timed_shape(one_launch):
    """Four packed batches of (256, 50, 1000) through the captured graph = without it = the launches it replaces, rank for rank, in either form."""
    B, T, NI, nb = 256, 50, 1000, 4
    P = orc.random_params(orc.bert4rec_param_shapes(N_ITEMS, HID), seed=77)
    eng = make_engine(P, T)
    cus = [{k: v.cuda() for k, v in eval_batch(B, T, NI, 900 + i).items()} for i in range(nb)]
    torch.cuda.synchronize()
    eng.EVAL_ONE_LAUNCH = one_launch
    pl = eng.plan(B, T, NI, need_grad=False)
    packed = torch.stack([eng.pack_batch(pl, *(c[k] for k in KEYS)) for c in cus])
    out_g = eng.eval_epoch(pl, packed, FIX, with_loss=True, use_graph=True)
    eng.sync()
    assert (FIX, True) in pl.eval_graphs
    out_e = eng.eval_epoch(pl, packed, FIX, with_loss=True, use_graph=False)
    eng.sync()
    assert torch.equal(out_g, out_e)
    for i, c in enumerate(cus):
        own, r, r0 = old_path(eng, pl, c)
        assert torch.equal(out_g[i, :B], r) and torch.equal(out_g[i, B:2 * B], r0), i
        want = torch.nn.functional.binary_cross_entropy(own.double(), c["label"].double(), reduction="none").sum(1) / (B * NI)
        got = out_g[i, 2 * B:].view(torch.float32).double()
        assert float((got - want).abs().max()) <= 1e-6 * float(want.abs().max()) + 1e-9


# ---------------------------------------------------------------------------- isDR and the comp models
@pytest.mark.parametrize("one_launch", FORMS)
def test_dr_model_evaluates_like_the_plain_one(one_launch):
    B, T, NI = 16, 50, 100
    P = orc.random_params(orc.bert4rec_param_shapes(N_ITEMS, HID, dr=True), seed=21)
    eng = make_engine(P, T, dr=True)
    pl = eng.plan(B, T, NI, need_grad=False)
    eng.EVAL_ONE_LAUNCH = True
    assert eng.eval_fused_ok(pl) and eng._eval_one_launch(pl)
    for seed, dom in ((50, None), (51, 1)):
        cu = {k: v.cuda() for k, v in eval_batch(B, T, NI, seed, dom).items()}
        torch.cuda.synchronize()
        check_against_old(eng, pl, cu, B, T, NI, one_launch)


@pytest.mark.parametrize("kind", ["inc", "itc"])
@pytest.mark.parametrize("B,T", [(32, 20), (8, 32)])
def test_comp_models_evaluate_staged_with_the_same_bits(kind, B, T, monkeypatch):
    NI = 100
    P = orc.random_params(orc.bert4rec_param_shapes(N_ITEMS, HID, inc_bs=B if kind == "inc" else 0, itc_bs=B if kind == "itc" else 0), seed=31)
    eng = make_engine(P, T, comp=kind, comp_bs=B, comp_threshold=1.0 / B)
    pl = eng.plan(B, T, NI, need_grad=False)
    assert pl.shape.Tenc == 2 * T
    eng.EVAL_ONE_LAUNCH = True
    assert eng.eval_fused_ok(pl) and not eng._eval_one_launch(pl)
    cu = {k: v.cuda() for k, v in eval_batch(B, T, NI, 60).items()}
    torch.cuda.synchronize()
    check_against_old(eng, pl, cu, B, T, NI, False)
    eng.load_batch(pl, *(cu[k] for k in KEYS))
    names = record_launches(monkeypatch, lambda: eng.enqueue_eval(pl, FIX, build_images=False))
    eng.sync()
    assert "amid_bert_comp_fwd_f32" in names and "amid_bert_seq_fwd_gather_infer_f32" not in names and "amid_head_fwd_f32" not in names


def test_comp_batch_that_is_not_bs_rows_still_raises():
    from amid_amd import model_seq
    T, bs = 20, 32
    model = model_seq.BERT4Rec(10, D, 200, D, T, 16, bs, True, False, 0.5, 0.5, seed=2)
    model.eval()
    b = eval_batch(8, T, 31, 5, n_items=200)
    ep = {k: v.cuda().unsqueeze(0) for k, v in b.items() if k != "label"}
    ep["label"] = b["label"].cuda()
    assert model.eval_ranks(ep, FIX) is None           # a data-parallel shard of a comp batch keeps forward() ...
    with pytest.raises(ValueError):                     # ... which raises what it always raised
        with torch.no_grad():
            model(None, ep["i_node"][0], ep["neg_samples"][0], ep["seq_d1"][0], ep["seq_d2"][0], None, None, False)


# ---------------------------------------------------------------------------- fallback
def test_shapes_outside_the_fused_evaluation_fall_back():
    P = orc.random_params(orc.bert4rec_param_shapes(N_ITEMS, HID), seed=4)
    eng = make_engine(P, 70)
    pl = eng.plan(4, 70, 5, need_grad=False)
    assert not eng.eval_fused_ok(pl)                  # T 70: no matrix-core attention over a live list
    with pytest.raises(ValueError):
        eng.enqueue_eval(pl, FIX)
    eng = make_engine(P, 20)
    pl = eng.plan(4, 20, 5, need_grad=False)
    assert eng.eval_fused_ok(pl)
    pl.strip = False                                  # a row-tile plan
    assert not eng.eval_fused_ok(pl)
    # comp over 2T = 80 tokens
    Pc = orc.random_params(orc.bert4rec_param_shapes(N_ITEMS, HID, inc_bs=4), seed=4)
    eng = make_engine(Pc, 40, comp="inc", comp_bs=4)
    assert not eng.eval_fused_ok(eng.plan(4, 40, 5, need_grad=False))


def test_eval_ranks_returns_none_beyond_64_tokens():
    from amid_amd import model_seq
    T, bs = 70, 4
    model = model_seq.BERT4Rec(10, D, 200, D, T, 16, bs, False, False, 0.5, 0.5, seed=2)
    model.eval()
    bt = [eval_batch(bs, T, 11, 5 + i, n_items=200) for i in range(2)]
    ep = {k: torch.stack([b[k] for b in bt]).cuda() for k in KEYS if k != "label"}
    ep["label"] = bt[0]["label"].cuda()
    assert model.eval_ranks(ep, FIX) is None


def test_eval_ranks_returns_none_on_a_row_tile_plan(monkeypatch):
    from amid_amd import model_seq
    from amid_amd.engine_bert import Bert4recEngine
    monkeypatch.setattr(Bert4recEngine, "STRIP_KERNELS", False)           # the block on csrc/bert.hip's row-tile kernels
    T, bs = 20, 4
    model = model_seq.BERT4Rec(10, D, 200, D, T, 16, bs, False, False, 0.5, 0.5, seed=2)
    model.eval()
    pl = model.engine.plan(bs, T, 11, need_grad=False)
    assert not pl.strip and not model.engine.eval_fused_ok(pl)
    bt = [eval_batch(bs, T, 11, 5 + i, n_items=200) for i in range(2)]
    ep = {k: torch.stack([b[k] for b in bt]).cuda() for k in KEYS if k != "label"}
    ep["label"] = bt[0]["label"].cuda()
    assert model.eval_ranks(ep, FIX) is None


# ---------------------------------------------------------------------------- end to end
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


def same_metrics(got, base):
    assert set(got) == set(base)
    for k, v in base.items():
        if k == "loss":
            assert abs(got[k] - v) <= 1e-6 * abs(v)
        else:
            assert got[k] == v or all(np.isnan(a) and np.isnan(b) or a == b for a, b in zip(got[k], v)), k


def test_module_eval_ranks_is_fused():
    from amid_amd import model_seq
    T, bs, NI = 20, 8, 31
    model = model_seq.BERT4Rec(10, D, 200, D, T, 16, bs, False, False, 0.5, 0.5, seed=2)
    model.eval()
    bt = [eval_batch(bs, T, NI, 5 + i, n_items=200) for i in range(3)]
    ep = {k: torch.stack([b[k] for b in bt]).cuda() for k in KEYS if k != "label"}
    ep["label"] = bt[0]["label"].cuda()
    out = model.eval_ranks(ep, FIX)
    assert out is not None
    assert out["rank"].shape == (3, bs) and out["rank_raw"].shape == (3, bs) and out["loss"].shape == (3,)
    assert bool(torch.isfinite(out["loss"]).all())


@pytest.mark.parametrize("one_launch", FORMS)
@pytest.mark.parametrize("overlap", [False, True])
def test_train_sr_test_gives_the_same_metrics_either_way(tmp_path, overlap, one_launch):
    """train_sr.test() through eval_ranks (one graph replay a batch, either form) and through model.forward + the rank kernel -- the path the
    parent took -- on the same evaluation set and negatives: the same metrics per split, the same loss to rounding."""
    import argparse
    from amid_amd import model_seq
    from amid_amd.dataset_seq import DeviceBatches, DualDomainSeqDataset
    from amid_amd.train_sr import test
    rng = np.random.default_rng(5)
    _write_csv(tmp_path / "toy_test.csv", 200, rng, 1, 400, 400, 900)
    ds = DualDomainSeqDataset(seq_len=20, isTrain=False, neg_nums=99, long_length=7, pad_id=1001, seed=3, csv_path=str(tmp_path / "toy_test.csv"))
    model = model_seq.BERT4Rec(10, D, 1100, D, 20, 32, 32, False, False, 0.5, 0.5, seed=2)
    args = argparse.Namespace(overlap=overlap)
    res = {}
    for fused, one in ((True, one_launch), (False, True)):
        model.engine.EVAL_FUSED, model.engine.EVAL_ONE_LAUNCH = fused, one
        model.engine.plan(32, 20, 100, need_grad=False).eval_graphs = {}      # (a graph captured in the other form)
        vb = DeviceBatches(ds, 32, shuffle=False, device="cuda:0", seed=9)
        res[(fused, one)] = test(model, args, vb)
    model.engine.EVAL_FUSED = model.engine.EVAL_ONE_LAUNCH = True
    same_metrics(res[(True, one_launch)], res[(False, True)])


@pytest.mark.parametrize("one_launch", FORMS)
def test_full_ranks_and_recommend_do_not_depend_on_the_switch(tmp_path, one_launch):
    """full_ranks and recommend take their user vectors from enqueue_user_vectors: pl.ev_u of the fused evaluation (either form), enqueue_forward's
    pl.u without it -- the same ranks, ids and scores, bitwise."""
    from amid_amd import model_seq
    from amid_amd.dataset_seq import DeviceBatches, DualDomainSeqDataset
    rng = np.random.default_rng(8)
    _write_csv(tmp_path / "toy_test.csv", 128, rng, 1, 60, 60, 119)
    ds = DualDomainSeqDataset(seq_len=20, isTrain=False, neg_nums=30, long_length=7, pad_id=119, seed=3, csv_path=str(tmp_path / "toy_test.csv"))
    bs = 32
    model = model_seq.BERT4Rec(10, D, 120, D, 20, 16, bs, False, False, 0.5, 0.5, seed=2)
    model.eval()
    g = torch.Generator().manual_seed(2)
    s1 = torch.randint(1, 60, (bs, 20), generator=g)
    s2 = torch.randint(60, 119, (bs, 20), generator=g)
    dom = torch.randint(0, 2, (bs,), generator=g)
    res = {}
    for fused, one in ((True, one_launch), (False, True)):
        model.engine.EVAL_FUSED, model.engine.EVAL_ONE_LAUNCH = fused, one
        vb = DeviceBatches(ds, bs, shuffle=False, device="cuda:0", seed=9)
        ep = vb.epoch_tensors()
        pl = model.engine.plan(bs, 20, 31, need_grad=False)
        assert model.engine.eval_fused_ok(pl) == fused
        fr = model.full_ranks(ep, vb, FIX)
        ids, scores = model.recommend(s1.cuda(), s2.cuda(), dom.cuda(), k=10)
        torch.cuda.synchronize()
        res[(fused, one)] = (fr["rank"].clone(), fr["rank_raw"].clone(), ids.clone(), scores.clone())
    model.engine.EVAL_FUSED = model.engine.EVAL_ONE_LAUNCH = True
    for a, b in zip(res[(True, one_launch)], res[(False, True)]):
        assert torch.equal(a, b), one_launch
    assert int(res[(False, True)][0].max()) > 0


def forward_loop_metrics(model, args, vb):
    """test()'s numbers the way the parent computed them for BERT4Rec: model.forward + the masked BCE + the rank kernel per batch (train_sr.py:55-64,
    :114-115), then the same metric code -- by switching the fused evaluation off, which leaves test() nothing but that loop."""
    from amid_amd.train_sr import test
    model.engine.EVAL_FUSED = False
    try:
        return test(model, args, vb)
    finally:
        model.engine.EVAL_FUSED = True


@pytest.mark.parametrize("case", ["T70", "row_tile"])
def test_train_sr_test_on_a_fallback_shape_gives_the_forward_loops_numbers(tmp_path, case, monkeypatch):
    """More than 64 encoder tokens / a row-tile plan: eval_ranks returns None inside test(), which then runs the loop it always ran -- the same
    metrics as with the fused evaluation switched off."""
    import argparse
    from amid_amd import model_seq
    from amid_amd.dataset_seq import DeviceBatches, DualDomainSeqDataset
    from amid_amd.engine_bert import Bert4recEngine
    from amid_amd.train_sr import test
    if case == "row_tile":
        monkeypatch.setattr(Bert4recEngine, "STRIP_KERNELS", False)
    T = 70 if case == "T70" else 20
    rng = np.random.default_rng(5)
    _write_csv(tmp_path / "toy_test.csv", 96, rng, 1, 400, 400, 900)
    ds = DualDomainSeqDataset(seq_len=T, isTrain=False, neg_nums=99, long_length=7, pad_id=1001, seed=3, csv_path=str(tmp_path / "toy_test.csv"))
    model = model_seq.BERT4Rec(10, D, 1100, D, T, 32, 32, False, False, 0.5, 0.5, seed=2)
    args = argparse.Namespace(overlap=True)
    assert model.engine.EVAL_FUSED and not model.engine.eval_fused_ok(model.engine.plan(32, T, 100, need_grad=False))
    calls = []
    orig = model.eval_ranks
    monkeypatch.setattr(model, "eval_ranks", lambda *a, **k: calls.append(orig(*a, **k)) or calls[-1])
    got = test(model, args, DeviceBatches(ds, 32, shuffle=False, device="cuda:0", seed=9))
    assert calls == [None]
    base = forward_loop_metrics(model, args, DeviceBatches(ds, 32, shuffle=False, device="cuda:0", seed=9))
    same_metrics(got, base)
    assert all(np.isfinite(v).all() for k, v in got.items() if k == "loss")
