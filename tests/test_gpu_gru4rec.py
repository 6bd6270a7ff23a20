"""GPU parity of the GRU4Rec path (engine_gru.Gru4recEngine, model_gru.GRU4Rec): the reference's own logits, loss and gradients (g16), the
nn.Module surface, train steps on an input pool against float64 Adam on tests/gru_ref.py, the fused evaluation against the launches it
replaces, full-catalog ranking / top-K, checkpoints, the two command lines, and what the model refuses."""
import os

import numpy as np
import pytest
import torch

from oracle import amid_oracle as orc
from tests import gru_ref
from tests.test_gpu_sasrec import GOLDEN, dense_table_grad, log, rel_l2, relmax

pytestmark = pytest.mark.gpu
D = 128
KEYS = ("i_node", "neg_samples", "seq_d1", "seq_d2", "label", "domain_id")


def make_engine(P, T, lr=5e-4, seed=0):
    from amid_amd.engine_gru import Gru4recEngine
    n_rows = P["item_emb_layer.emb_item.weight"].shape[0]
    hid = P["predictModule.fc.0.weight"].shape[0]
    eng = Gru4recEngine(n_rows, D, T, hid, lr=lr, seed=seed)
    eng.load_state_dict(P)
    return eng


def make_model(n_items, T, hid, bs, **kw):
    from amid_amd.model_gru import GRU4Rec
    return GRU4Rec(10, D, n_items, D, T, hid, bs, False, False, 0.5, 0.5, **kw)


def golden():
    z = np.load(os.path.join(GOLDEN, "g16_gru4rec.npz"))
    B = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("B/")}
    B["label"] = torch.from_numpy(z["labels"])
    G = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("G/")}
    return z, gru_ref.golden_params(z), B, G


def grads_check(tag, eng, pl, grads, tol, l2tol):
    """tests/test_gpu_bert4rec.py's comparison: every dense gradient and the table's (through the dense view of the step's unique rows)."""
    bad = []
    for name in eng.dense.slots:
        got = eng.dense.view(name, eng.dense.grad)
        e, e2 = relmax(got, grads[name]), rel_l2(got, grads[name])
        log(f"{tag} grad {name:30s} relmax {e:.3e} l2 {e2:.3e}")
        if not (e < tol and e2 < l2tol):
            bad.append((name, e, e2))
    assert not bad, bad
    tg = dense_table_grad(eng, pl)
    e, e2 = relmax(tg, grads["item_emb_layer.emb_item.weight"]), rel_l2(tg, grads["item_emb_layer.emb_item.weight"])
    log(f"{tag} grad table relmax {e:.3e} l2 {e2:.3e}")
    assert e < tol and e2 < l2tol, (e, e2)


# ---------------------------------------------------------------------------- 1. the reference's own numbers
def test_golden_forward_loss_and_grads():
    """Engine forward and backward on g16 at the bars of test_forward_golden_bert4rec_eval / test_backward_golden_bert4rec_grads."""
    z, P, B, G = golden()
    Bn, T = B["seq_d1"].shape
    eng = make_engine(P, T)
    pl = eng.plan(Bn, T, 2, need_grad=True)
    cu = {k: v.cuda() for k, v in B.items()}
    eng.load_batch(pl, *(cu[k] for k in KEYS))
    eng.enqueue_prepare(pl, sparse=True)
    eng.enqueue_forward(pl, train=False, with_loss=True)
    eng.enqueue_backward(pl, train=False)
    eng.sync()
    eng.check_index_error(pl)
    e1, e2 = relmax(pl.p1, z["p1"]), relmax(pl.p2, z["p2"])
    log(f"golden g16 gru4rec: logits {e1:.3e} {e2:.3e} loss {float(pl.loss.item()):.7f} / {float(z['loss']):.7f}")
    assert e1 < 1e-4 and e2 < 1e-4
    assert abs(float(pl.loss.item()) - float(z["loss"])) < 1e-5
    grads_check("golden g16 gru4rec", eng, pl, G, 5e-4, 5e-4)
    pad = int(z["n_items"]) - 1                       # the pad id's row is an ordinary trained row
    assert float(dense_table_grad(eng, pl)[pad].abs().max()) > 0


# ---------------------------------------------------------------------------- 2. the nn.Module surface
def test_module_surface_autograd_and_train_step():
    """state_dict keys and shapes as the reference's; forward gives the golden's logits in train() and eval() alike (one GRU layer: no
    dropout); loss.backward() fills .grad with the golden's gradients; the fused train_step() on a twin -- the live sequences only, head
    forward + backward fused -- computes the same gradients.  Twin bar 5e-5 of a tensor's largest entry: both sum the same fp32 products;
    the live walk regroups at most B T = 60 rows per sum, each regrouping worth <= 2^-24 of the sum of magnitudes (a few times the largest
    entry), and the fused head adds its B partials in another order."""
    z, P, B, G = golden()
    Bn, T = B["seq_d1"].shape
    n_items, hid = int(z["n_items"]), int(z["hid"])
    cu = {k: v.cuda() for k, v in B.items()}
    m = make_model(n_items, T, hid, Bn, lr=1e-3, seed=5)
    sd = m.state_dict()
    assert list(sd) == list(gru_ref.gru4rec_param_shapes(n_items, D, hid))
    assert all(tuple(sd[k].shape) == s for k, s in gru_ref.gru4rec_param_shapes(n_items, D, hid).items())
    assert float(sd["gru1.weight_hh_l0"].abs().max()) <= 1.0 / D ** 0.5 and float(sd["gru2.bias_ih_l0"].abs().max()) > 0      # nn.GRU's init
    m.load_state_dict(P, strict=True)
    outs = {}
    for mode in ("eval", "train"):
        getattr(m, mode)()
        with torch.no_grad():
            outs[mode] = [o.clone() for o in m(None, cu["i_node"], cu["neg_samples"], cu["seq_d1"], cu["seq_d2"], None, None)]
    assert torch.equal(outs["eval"][0], outs["train"][0]) and torch.equal(outs["eval"][1], outs["train"][1])
    assert relmax(outs["eval"][0], z["p1"]) < 1e-4 and relmax(outs["eval"][1], z["p2"]) < 1e-4
    p1, p2 = m(None, cu["i_node"], cu["neg_samples"], cu["seq_d1"], cu["seq_d2"], None, None)
    crit = torch.nn.BCELoss(reduction="none")
    dom = cu["domain_id"].unsqueeze(1).float()
    loss = torch.mean(crit(p1, cu["label"]) * (1 - dom) + crit(p2, cu["label"]) * dom)            # train_sr.py:203-212
    loss.backward()
    assert abs(float(loss.detach()) - float(z["loss"])) < 1e-5
    auto = {k: v.grad.detach().cpu().clone() for k, v in m.named_parameters()}
    for k, g in G.items():
        assert relmax(auto[k], g) < 5e-4 and rel_l2(auto[k], g) < 5e-4, k
    twin = make_model(n_items, T, hid, Bn, lr=1e-3, seed=6)
    twin.load_state_dict(P, strict=True)
    twin.train_step(*(cu[k] for k in KEYS), use_graph=False)
    eng, pl = twin.engine, twin._last_plan
    eng.sync()
    assert abs(float(pl.loss.item()) - float(z["loss"])) < 1e-5
    fused = {name: eng.dense.view(name, eng.dense.grad).cpu().clone() for name in eng.dense.slots}
    fused["item_emb_layer.emb_item.weight"] = dense_table_grad(eng, pl)
    for k in G:
        e = relmax(fused[k], auto[k])
        log(f"gru4rec train_step vs autograd {k:30s} relmax {e:.3e}")
        assert e < 5e-5, (k, e)


# ---------------------------------------------------------------------------- 3. train steps
@pytest.mark.parametrize("compact", [False, True])
def test_five_pool_steps_track_fp64_adam(compact):
    """Five train_step()s on an input pool -- graph replay, the live sequences only -- against five float64 torch.optim.Adam steps of
    tests/gru_ref.py on the same batches: every parameter within 1e-4; table rows no batch touches keep their bits.  compact: the sparse
    side on the live sequences' positions only, what the engine does from 65 536 indices a step on (COMPACT_MIN_IDX), forced here."""
    n_items, T, hid, Bn, K, lr = 400, 20, 16, 24, 5, 1e-3
    P = orc.random_params(gru_ref.gru4rec_param_shapes(n_items, D, hid), seed=77)
    batches = [orc.synthetic_batch(Bn, T, 300, pad_id=n_items - 1, neg=1, seed=900 + t) for t in range(K)]      # ids 1 .. 299 and the pad
    m = make_model(n_items, T, hid, Bn, lr=lr, seed=1)
    m.load_state_dict(P, strict=True)
    if compact:
        m.engine.COMPACT_MIN_IDX = 0
    ep = {k: torch.stack([b[k] for b in batches]).cuda() for k in ("i_node", "neg_samples", "seq_d1", "seq_d2", "domain_id")}
    ep["label"] = batches[0]["label"].cuda()
    assert m.begin_epoch_pool(ep) == K
    eng, pl = m.engine, m._pool_plan
    losses = []
    for _ in range(K):
        loss = m.pool_step()
        eng.sync()                     # (pool_step() returns without making torch's stream wait for the engine's)
        losses.append(float(loss.item()))
    m.end_epoch_pool()
    assert eng.has_graph(pl) and eng.live_forward_ok(pl) and bool(pl.compact) == compact
    leaves = {k: v.double().clone().requires_grad_(True) for k, v in P.items()}
    opt = torch.optim.Adam(list(leaves.values()), lr=lr)
    for t, b in enumerate(batches):
        opt.zero_grad()
        p1, p2 = gru_ref.gru4rec_forward(leaves, b["i_node"], b["neg_samples"], b["seq_d1"], b["seq_d2"])
        loss = orc.masked_bce_loss(p1, p2, b["label"].double(), b["domain_id"])
        loss.backward()
        opt.step()
        assert abs(losses[t] - float(loss.detach())) < 1e-4, (t, losses[t], float(loss.detach()))
    sd = m.state_dict()
    worst = 0.0
    for k, v in leaves.items():
        d = float((sd[k].detach().cpu().double() - v.detach()).abs().max())
        worst = max(worst, d)
        assert d < 1e-4, (k, d)
    log(f"gru4rec pool steps: worst |param diff| to fp64 Adam after {K} steps {worst:.3e}")
    idle = torch.arange(300, n_items - 1)
    assert torch.equal(sd["item_emb_layer.emb_item.weight"].cpu()[idle], P["item_emb_layer.emb_item.weight"][idle])
    assert not torch.equal(sd["item_emb_layer.emb_item.weight"].cpu()[n_items - 1], P["item_emb_layer.emb_item.weight"][n_items - 1])


# ---------------------------------------------------------------------------- 4. evaluation
EVAL_SHAPES = [(1, 1, 2), (7, 17, 5), (16, 50, 100), (33, 20, 1000)]


@pytest.mark.parametrize("B,T,NI", EVAL_SHAPES)
def test_eval_batch_is_bit_identical_to_the_forward_and_rank_kernels(B, T, NI):
    """enqueue_eval (marshal + live list, the live rows gathered, projection + inference recurrence over the list, amid_eval_head_f32)
    gives the bits of enqueue_forward(train=False) over both domains + the rank kernel: x[2]'s live rows, the scores, both ranks; the loss
    parts to 1e-6 (as tests/test_gpu_bert_eval.py holds BERT4Rec's)."""
    from tests.test_gpu_bert_eval import FIX, N_ITEMS, HID, eval_batch, live_rows, old_path, poison
    P = orc.random_params(gru_ref.gru4rec_param_shapes(N_ITEMS, D, HID), seed=3 + T)
    eng = make_engine(P, T)
    pl = eng.plan(B, T, NI, need_grad=False)
    assert eng.eval_fused_ok(pl)
    for seed, dom in ((40, None), (41, 0), (42, 1)):
        cu = {k: v.cuda() for k, v in eval_batch(B, T, NI, seed, dom).items()}
        torch.cuda.synchronize()          # (the engine's stream does not wait for torch's)
        own, r, r0 = old_path(eng, pl, cu)
        x_old = live_rows(pl.x[2].clone(), cu, B, T)
        poison(eng, pl)
        pl.gi.fill_(float("nan"))
        torch.cuda.synchronize()
        eng.load_batch(pl, *(cu[k] for k in KEYS))
        eng.enqueue_eval(pl, FIX, with_loss=True, want_scores=True)
        eng.sync()
        eng.check_index_error(pl)
        assert bool(torch.isfinite(x_old).all()) and torch.equal(live_rows(pl.x[2].clone(), cu, B, T), x_old)
        assert torch.equal(pl.ev_p, own), float((pl.ev_p - own).abs().max())
        assert torch.equal(pl.ev_rank, r) and torch.equal(pl.ev_rank_raw, r0)
        want = torch.nn.functional.binary_cross_entropy(own.double(), cu["label"].double(), reduction="none").sum(1) / (B * NI)
        assert float((pl.ev_loss_part.double() - want).abs().max()) <= 1e-6 * float(want.abs().max()) + 1e-9


def test_eval_epoch_graph_equals_eager_and_scores_follow_the_helper():
    from tests.test_gpu_bert_eval import FIX, eval_batch
    n_items, hid, B, T, NI, n = 500, 16, 17, 20, 30, 3
    P = orc.random_params(gru_ref.gru4rec_param_shapes(n_items, D, hid), seed=9)
    eng = make_engine(P, T)
    pl = eng.plan(B, T, NI, need_grad=False)
    bs = [eval_batch(B, T, NI, 60 + i, n_items=n_items) for i in range(n)]
    cu = [{k: v.cuda() for k, v in b.items()} for b in bs]
    torch.cuda.synchronize()
    packed = torch.stack([eng.pack_batch(pl, *(c[k] for k in KEYS)) for c in cu])
    eng.sync()
    out = {}
    for use_graph in (True, False):
        res = eng.eval_epoch(pl, packed, FIX, use_graph=use_graph)
        eng.sync()                     # (nothing is synchronised inside: the results are the engine stream's)
        out[use_graph] = res.clone()
    out_g, out_e = out[True], out[False]
    assert torch.equal(out_g, out_e) and int(out_g[:, :B].max()) > 0
    # the last batch's own-domain scores against the float64 helper, at the logits' bar
    eng.load_batch(pl, *(cu[-1][k] for k in KEYS))
    eng.enqueue_eval(pl, FIX, with_loss=True, want_scores=True)
    eng.sync()
    b = bs[-1]
    with torch.no_grad():
        p1, p2 = gru_ref.gru4rec_forward({k: v.double() for k, v in P.items()}, b["i_node"], b["neg_samples"], b["seq_d1"], b["seq_d2"])
    want = torch.where(b["domain_id"][:, None] != 0, p2, p1)
    assert relmax(pl.ev_p, want) < 1e-4


def _write_csv(path, n, rng, lo1, hi1, lo2, hi2):
    from tests.test_gpu_module import _write_csv as w
    w(path, n, rng, lo1, hi1, lo2, hi2)


def test_full_ranks_recommend_and_recommend_all_agree(tmp_path):
    """As tests/test_gpu_eval_long.py section 7 on a small table: the full-catalog ranks recounted on the host from recommend()'s scores of
    every table row, rank_full >= rank_sampled, and recommend_all's batches are recommend()'s, bit for bit."""
    from amid_amd.dataset_seq import DeviceBatches, DualDomainSeqDataset
    from tests.test_gpu_bert_eval import FIX
    n_items, bs, neg, T = 120, 32, 30, 20
    _write_csv(tmp_path / "toy_test.csv", 64, np.random.default_rng(5), 1, 60, 60, 119)
    ds = DualDomainSeqDataset(seq_len=T, isTrain=False, neg_nums=neg, long_length=7, pad_id=119, seed=3, csv_path=str(tmp_path / "toy_test.csv"))
    model = make_model(n_items, T, 32, bs, seed=2)
    model.eval()
    vb = DeviceBatches(ds, bs, shuffle=False, device="cuda:0", seed=9)
    ep = vb.epoch_tensors()
    sampled = model.eval_ranks(ep, FIX)
    assert sampled is not None
    fr = model.full_ranks(ep, vb, FIX)
    assert bool((fr["rank"] >= sampled["rank"]).all()) and bool((fr["rank_raw"] >= sampled["rank_raw"]).all()) and int(fr["rank"].max()) > 0
    ids, sc = model.recommend(ep["seq_d1"][0], ep["seq_d2"][0], ep["domain_id"][0], k=n_items, exclude_history=False)
    torch.cuda.synchronize()
    ids_c, sc_c = ids.cpu(), sc.cpu()
    dom, pos = ep["domain_id"][0].cpu(), ep["i_node"][0].cpu()
    for b in range(bs):
        assert sorted(ids_c[b].tolist()) == list(range(n_items))
        score = torch.empty(n_items)
        score[ids_c[b]] = sc_c[b]
        cand = sorted(set(ds.pool[int(dom[b])].tolist()) - set(ds.own_items[b].tolist()))
        cs = score[torch.tensor(cand, dtype=torch.long)]
        assert int((cs > score[int(pos[b])] - torch.tensor(FIX, dtype=torch.float32)).sum()) == int(fr["rank"][0, b]), b
        assert int((cs > score[int(pos[b])]).sum()) == int(fr["rank_raw"][0, b]), b
    all_i, all_s = model.recommend_all(ep, k=10)
    for i in range(ep["seq_d1"].shape[0]):
        one_i, one_s = model.recommend(ep["seq_d1"][i], ep["seq_d2"][i], ep["domain_id"][i], k=10)
        assert torch.equal(all_i[i], one_i) and torch.equal(all_s[i], one_s), i
        hist = torch.where(ep["domain_id"][i][:, None] != 0, ep["seq_d2"][i], ep["seq_d1"][i])
        assert not bool((one_i[:, :, None] == hist[:, None, :]).any())


# ---------------------------------------------------------------------------- 5. checkpoint
def test_resumed_run_is_the_uninterrupted_run(tmp_path):
    """k steps, save, m steps; a model of another seed loads the file and takes the same m steps: the losses and the whole training state, bit for bit."""
    from tests.test_gpu_checkpoint import B as CB, N_ITEMS as CN, T as CT, _assert_same, _epoch, _flushed_state, _steps
    ep = _epoch(7, seed=11, hot=(5,))
    a = make_model(CN, CT, 16, CB, lr=1e-3, seed=3)
    _steps(a, ep, range(3))
    path = str(tmp_path / "state.pt")
    a.save_training_state(path, epoch=1)
    la = _steps(a, ep, range(3, 7))
    b = make_model(CN, CT, 16, CB, lr=1e-3, seed=4)
    assert b.load_training_state(path) == {"epoch": 1}
    lb = _steps(b, ep, range(3, 7))
    assert len(la) == len(lb) == 4
    for x, y in zip(la, lb):
        assert torch.equal(x, y)
    _assert_same(_flushed_state(a), _flushed_state(b))
    from amid_amd.model_seq import BERT4Rec
    with pytest.raises(ValueError):                  # another model's state does not fit
        BERT4Rec(10, 128, CN, 128, CT, 16, CB, False, False, 0.5, 0.5, seed=1).load_training_state(path)


# ---------------------------------------------------------------------------- 6. the command lines
def test_cli_train_then_recommend(tmp_path):
    from amid_amd import recommend, train_sr
    from amid_amd.dataset_seq import DualDomainSeqDataset
    rng = np.random.default_rng(0)
    root = tmp_path / "amazon_dataset"
    root.mkdir()
    _write_csv(root / "toy_train75.csv", 300, rng, 1, 400, 400, 900)
    _write_csv(root / "toy_test.csv", 80, rng, 1, 400, 400, 900)
    common = ["--data_root", str(tmp_path), "-ds", "amazon", "-dm", "toy", "--overlap_ratio", "0.75", "--model", "gru4rec", "--bs", "32",
              "--seq_len", "20", "--emb_dim", "128", "--hid_dim", "16", "--neg_nums", "19"]
    summary = train_sr.main(common + ["--epoch", "2", "--seeds", "1", "-md", str(tmp_path / "model"), "--save_dir", str(tmp_path / "run")])
    assert len(summary) == 1
    best = summary[0]
    assert ("d1", "HR@10") in best and ("d2", "MRR") in best and all(0.0 <= v <= 1.0 for v in best.values())
    assert (tmp_path / "model" / "log0.txt").exists()
    K = 10
    res = recommend.main(common + ["--weights", str(tmp_path / "run" / "seed0" / "best_d1.pt"), "--topk", str(K), "--out", str(tmp_path / "top.npz")])
    z = np.load(tmp_path / "top.npz")
    pad = 447410 + 1
    ds = DualDomainSeqDataset(seq_len=20, isTrain=False, neg_nums=19, long_length=7, pad_id=pad, seed=1000, csv_path=str(root / "toy_test.csv"))
    items, scores = z["items"], z["scores"]
    assert items.shape == (80, K) and scores.shape == (80, K) and bool((items >= 0).all())
    assert np.array_equal(res["items"], items) and bool((scores[:, 1:] <= scores[:, :-1]).all())
    for r in range(80):
        d = int(ds.domain_id[r] != 0)
        assert len(set(items[r].tolist())) == K
        assert not set(items[r].tolist()) & set((ds.seq_d2 if d else ds.seq_d1)[r].tolist()), r


# ---------------------------------------------------------------------------- 7. staying out
def test_refusals():
    from amid_amd import model_seq
    from amid_amd.model_gru import GRU4Rec
    for kw in (dict(isInC=True), dict(isItC=True), dict(isDR=True), dict(compute="bf16")):
        a = dict(isInC=False, isItC=False, isDR=False)
        a.update(kw)
        with pytest.raises(ValueError):
            GRU4Rec(10, 128, 100, 128, 20, 32, 4, a.pop("isInC"), a.pop("isItC"), 0.5, 0.5, **a)
    with pytest.raises(ValueError):
        GRU4Rec(10, 64, 100, 64, 20, 32, 4, False, False, 0.5, 0.5)
    with pytest.raises(NotImplementedError, match="model_gru"):
        model_seq.GRU4Rec(10, 128, 100, 128, 20, 32, 4, False, False, 0.5, 0.5)

    class World2:
        world = 2
    m = GRU4Rec(10, 128, 100, 128, 20, 32, 4, False, False, 0.5, 0.5)
    z = torch.zeros(4, dtype=torch.long, device="cuda")
    with pytest.raises(NotImplementedError):
        m.train_step(z, z.view(4, 1), z.view(4, 1).repeat(1, 20), z.view(4, 1).repeat(1, 20), torch.zeros(4, 2, device="cuda"), z, exchange=World2())
