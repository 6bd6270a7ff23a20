"""GPU parity of GRU4Rec with isInC / isItC / isDR (engine_gru.Gru4recEngine with inc_bs / itc_bs / dr, model_gru.GRU4RecAMID): the
reference's own outputs, losses and gradients (g17 isItC, g18 isInC, g19 all three under both objectives), the nn.Module surface, shape
edges against the float64 restatement tests/gru_amid_ref.py (pinned to the reference by tests/test_gru_amid_ref_golden.py), pool steps
on two Adam states against float64 Adam, the fused evaluation against the launches it replaces, serving, checkpoints, the command lines,
and what stays refused."""
import functools

import numpy as np
import pytest
import torch

from oracle import amid_oracle as orc
from tests import gru_amid_ref as ref
from tests.test_gpu_sasrec import dense_table_grad, log, rel_l2, relmax

pytestmark = pytest.mark.gpu
D = 128
KEYS = ("i_node", "neg_samples", "seq_d1", "seq_d2", "label", "domain_id")
OUTS = ("p1", "p2", "ips1", "ips2", "g1", "g2")
VARIANTS = {"itc": dict(isItC=True), "inc": dict(isInC=True), "inc_itc": dict(isInC=True, isItC=True), "itc_dr": dict(isItC=True, isDR=True)}


def full_flags(fl):
    out = dict(isInC=False, isItC=False, isDR=False, threshold1=0.5, threshold2=0.5)
    out.update(fl)
    return out


def make_engine(P, T, bs, fl, lr=5e-4, seed=0, dr_e_w=0.1):
    from amid_amd.engine_gru import Gru4recEngine
    fl = full_flags(fl)
    n_rows = P["item_emb_layer.emb_item.weight"].shape[0]
    hid = P["predictModule.fc.0.weight"].shape[0]
    eng = Gru4recEngine(n_rows, D, T, hid, lr=lr, seed=seed, itc_bs=bs if fl["isItC"] else 0, itc_threshold=fl["threshold2"],
                        inc_bs=bs if fl["isInC"] else 0, inc_threshold=fl["threshold1"], dr=fl["isDR"], dr_e_w=dr_e_w)
    eng.load_state_dict(P)
    return eng


def make_model(n_items, T, hid, bs, fl, **kw):
    from amid_amd.model_gru import GRU4RecAMID
    fl = full_flags(fl)
    return GRU4RecAMID(10, D, n_items, D, T, hid, bs, fl["isInC"], fl["isItC"], fl["threshold1"], fl["threshold2"], isDR=fl["isDR"], **kw)


def grads_check(tag, eng, pl, grads, tol, l2tol):
    bad = []
    for name in eng.dense.slots:
        got = eng.dense.view(name, eng.dense.grad)
        e, e2 = relmax(got, grads[name]), rel_l2(got, grads[name])
        log(f"{tag} grad {name:30s} relmax {e:.3e} l2 {e2:.3e}")
        if not (e < tol and e2 < l2tol):
            bad.append((name, e, e2))
    tg = dense_table_grad(eng, pl)
    e, e2 = relmax(tg, grads["item_emb_layer.emb_item.weight"]), rel_l2(tg, grads["item_emb_layer.emb_item.weight"])
    log(f"{tag} grad table relmax {e:.3e} l2 {e2:.3e}")
    if not (e < tol and e2 < l2tol):
        bad.append(("table", e, e2))
    assert not bad, bad


def run_engine(eng, batch, mode=0, need_grad=True):
    """Forward with loss (+ backward) of one batch through the engine's own launches; returns the plan."""
    Bn, T = batch["seq_d1"].shape
    pl = eng.plan(Bn, T, batch["label"].shape[1], need_grad=need_grad)
    cu = {k: v.cuda() for k, v in batch.items()}
    torch.cuda.synchronize()
    if eng.dr:
        eng.dr_mode = mode
    eng.load_batch(pl, *(cu[k] for k in KEYS), *((cu["ob_label"],) if eng.dr else ()))
    eng.enqueue_prepare(pl, sparse=need_grad)
    eng.enqueue_forward(pl, train=False, with_loss=True)
    if need_grad:
        eng.enqueue_backward(pl, train=False)
    eng.sync()
    eng.check_index_error(pl)
    return pl


def engine_outs(eng, pl):
    return (pl.p1, pl.p2) + ((pl.ips1, pl.ips2, pl.g1, pl.g2) if eng.dr else ())


# ---------------------------------------------------------------------------- 1. the reference's own numbers
@pytest.mark.parametrize("name,mode", [("g17_gru4rec_itc", 0), ("g18_gru4rec_inc", 0), ("g19_gru4rec_inc_itc_dr", 0), ("g19_gru4rec_inc_itc_dr", 1)])
def test_golden_forward_loss_and_grads(name, mode):
    """Engine forward, loss and backward on g17 / g18 / g19 at the bars test_gpu_gru4rec.py holds g16 to."""
    z, P, batch = ref.load_golden(name)
    fl = ref.golden_flags(z)
    Bn, T = batch["seq_d1"].shape
    eng = make_engine(P, T, Bn, fl, dr_e_w=float(z["dr_e_w"]) if fl["isDR"] else 0.1)
    pl = run_engine(eng, batch, mode)
    for got, k in zip(engine_outs(eng, pl), OUTS):
        e = relmax(got, z[k])
        log(f"golden {name} mode {mode}: {k} {e:.3e}")
        assert e < 1e-4, (k, e)
    if fl["isDR"]:
        lc, le, lr_ = (float(v) for v in pl.dr_losses.cpu())
        assert abs(lc - float(z["loss_cls"])) < 1e-5 and abs(le - float(z["loss_dr_e"])) < 1e-5 and abs(lr_ - float(z["loss_dr_r"])) < 1e-5
        pre = "GE/" if mode == 0 else "GR/"
    else:
        assert abs(float(pl.loss.item()) - float(z["loss"])) < 1e-5
        pre = "G/"
    G = {k[len(pre):]: torch.from_numpy(z[k]) for k in z if k.startswith(pre)}
    grads_check(f"golden {name} mode {mode}", eng, pl, G, 5e-4, 5e-4)


# ---------------------------------------------------------------------------- 2. the nn.Module surface
def torch_loss(outs, cu, z, fl):
    """The reference's objectives written with torch ops (train_sr.py:203-212; train_sr_dr.py:216-221)."""
    crit = torch.nn.BCELoss(reduction="none")
    dom = cu["domain_id"].unsqueeze(1).float()
    b1, b2 = crit(outs[0], cu["label"]), crit(outs[1], cu["label"])
    cls = torch.mean(b1 * (1 - dom) + b2 * dom)
    if not fl["isDR"]:
        return cls
    dr_e = torch.mean((b1 - outs[4]) ** 2 / outs[2] * (1 - dom) + (b2 - outs[5]) ** 2 / outs[3] * dom)
    return cls + float(z["dr_e_w"]) * dr_e


@pytest.mark.parametrize("name", ["g17_gru4rec_itc", "g18_gru4rec_inc", "g19_gru4rec_inc_itc_dr"])
def test_module_surface_autograd_and_train_step(name):
    """state_dict keys and shapes as the restatement's; train() and eval() give the same bits; loss.backward() fills .grad with the
    golden's gradients; the fused train_step() on a twin stays within 5e-5 of autograd per tensor (the plain model's twin bar)."""
    z, P, batch = ref.load_golden(name)
    fl = ref.golden_flags(z)
    Bn, T = batch["seq_d1"].shape
    n_items, hid = int(z["n_items"]), int(z["hid"])
    cu = {k: v.cuda() for k, v in batch.items()}
    m = make_model(n_items, T, hid, Bn, fl, lr=1e-3, seed=5)
    shapes = ref.gru4rec_amid_param_shapes(n_items, D, hid, Bn, fl["isInC"], fl["isItC"], fl["isDR"])
    sd = m.state_dict()
    assert list(sd) == list(shapes) and all(tuple(sd[k].shape) == s for k, s in shapes.items())
    m.load_state_dict(P, strict=True)
    if fl["isDR"]:
        m.engine.dr_e_w = float(z["dr_e_w"])
    outs = {}
    for mode in ("eval", "train"):
        getattr(m, mode)()
        with torch.no_grad():
            outs[mode] = [o.clone() for o in m(None, cu["i_node"], cu["neg_samples"], cu["seq_d1"], cu["seq_d2"], None, None)]
    assert len(outs["eval"]) == (6 if fl["isDR"] else 2)
    for a, b, k in zip(outs["eval"], outs["train"], OUTS):
        assert torch.equal(a, b) and relmax(a, z[k]) < 1e-4, k
    o = m(None, cu["i_node"], cu["neg_samples"], cu["seq_d1"], cu["seq_d2"], None, None)
    loss = torch_loss(o, cu, z, fl)
    loss.backward()
    want = float(z["loss_cls"]) + float(z["dr_e_w"]) * float(z["loss_dr_e"]) if fl["isDR"] else float(z["loss"])
    assert abs(float(loss.detach()) - want) < 1e-5
    pre = "GE/" if fl["isDR"] else "G/"
    G = {k[len(pre):]: torch.from_numpy(z[k]) for k in z if k.startswith(pre)}
    auto = {k: v.grad.detach().cpu().clone() for k, v in m.named_parameters()}
    for k, g in G.items():
        assert relmax(auto[k], g) < 5e-4 and rel_l2(auto[k], g) < 5e-4, k
    twin = make_model(n_items, T, hid, Bn, fl, lr=1e-3, seed=6)
    twin.load_state_dict(P, strict=True)
    if fl["isDR"]:
        twin.engine.dr_e_w = float(z["dr_e_w"])
    twin.train_step(*(cu[k] for k in KEYS), use_graph=False, **(dict(ob_label=cu["ob_label"], dr_objective=0) if fl["isDR"] else {}))
    eng, pl = twin.engine, twin._last_plan
    eng.sync()
    fused = {n: eng.dense.view(n, eng.dense.grad).cpu().clone() for n in eng.dense.slots}
    fused["item_emb_layer.emb_item.weight"] = dense_table_grad(eng, pl)
    for k in G:
        e = relmax(fused[k], auto[k])
        log(f"gru4rec amid {name} train_step vs autograd {k:30s} relmax {e:.3e}")
        assert e < 5e-5, (k, e)


# ---------------------------------------------------------------------------- 3. shape edges against the float64 restatement
N_EDGE, HID_EDGE = 200, 16


def pick_threshold(softmaxes):
    """The midpoint of the widest gap between neighbouring values that leaves every gate a row on and a row off; (threshold, margin)."""
    vals = torch.sort(torch.cat([s.double() for s in softmaxes])).values
    best = None
    for lo, hi in zip(vals[:-1].tolist(), vals[1:].tolist()):
        thr = 0.5 * (lo + hi)
        if all(bool((s > thr).any()) and bool((s <= thr).any()) for s in softmaxes):
            margin = min(float((s.double() - thr).abs().min()) for s in softmaxes)
            if best is None or margin > best[1]:
                best = (thr, margin)
    return best


def thresholds_for(P, batch, fl):
    """threshold1 / threshold2 from the float64 softmax of the case, each with its margin; None where no threshold splits a gate."""
    P64 = {k: v.double() for k, v in P.items()}
    fl = full_flags(fl)
    args = (batch["i_node"], batch["neg_samples"], batch["seq_d1"], batch["seq_d2"])
    margins = []
    if fl["isInC"]:
        taps = {}
        ref.gru4rec_amid_forward(P64, *args, isInC=True, taps=taps)
        got = pick_threshold([taps["inc_d1"]["softmax"], taps["inc_d2"]["softmax"]])
        if got is None:
            return None
        fl["threshold1"] = got[0]
        margins.append(got[1] / got[0])
    if fl["isItC"]:
        taps = {}
        ref.gru4rec_amid_forward(P64, *args, isInC=fl["isInC"], isItC=True, threshold1=fl["threshold1"], taps=taps)
        got = pick_threshold([taps["itc_d1"]["softmax"]])
        if got is None:
            return None
        fl["threshold2"] = got[0]
        margins.append(got[1] / got[0])
    return fl, min(margins)


@functools.lru_cache(maxsize=None)
def edge_case(variant, Bn, T):
    """(P, batch, flags with thresholds) of a shape-edge case: mixed domains, un-padded sequences, the first seed whose gates split with a
    margin of at least 1e-3 of the threshold (chosen here, on the CPU, from float64: no case is skipped)."""
    base = dict(VARIANTS[variant])
    shapes = ref.gru4rec_amid_param_shapes(N_EDGE, D, HID_EDGE, Bn, base.get("isInC", False), base.get("isItC", False), base.get("isDR", False))
    for seed in range(1000 * Bn + 10 * T, 1000 * Bn + 10 * T + 40):
        P = orc.random_params(shapes, seed=seed)
        ref.scale_params(P, 0.25, 2.0)
        g = torch.Generator().manual_seed(seed)
        dom = torch.arange(Bn) % 2 if Bn > 1 else torch.zeros(1, dtype=torch.long)
        batch = dict(i_node=torch.randint(1, N_EDGE, (Bn,), generator=g), neg_samples=torch.randint(1, N_EDGE, (Bn, 1), generator=g),
                     seq_d1=torch.randint(0, N_EDGE, (Bn, T), generator=g), seq_d2=torch.randint(0, N_EDGE, (Bn, T), generator=g),
                     domain_id=dom[torch.randperm(Bn, generator=g)].long(), ob_label=(torch.rand(Bn, generator=g) < 0.6).long())
        batch["label"] = torch.zeros(Bn, 2)
        batch["label"][:, 0] = 1.0
        got = thresholds_for(P, batch, base)
        if got is not None and got[1] >= 1e-3:
            return P, batch, got[0], got[1]
    raise AssertionError(f"no seed gives {variant} B {Bn} T {T} a gate margin of 1e-3 of the threshold")


@pytest.mark.parametrize("T", [1, 3, 20])
@pytest.mark.parametrize("Bn", [5, 16, 17, 32, 33])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_shape_edges_against_fp64(variant, Bn, T):
    """Outputs, loss and every gradient at the recurrence's 16-sequence tile edge and the mix kernels' dispatch edge (32 rows), at the
    golden tests' bars."""
    P, batch, fl, margin = edge_case(variant, Bn, T)
    assert margin >= 1e-3 and 0 < int(batch["domain_id"].sum()) < Bn
    which = "e" if fl["isDR"] else ""
    loss, outs, grads = ref.loss_and_grads(P, batch, which=which, **fl)
    eng = make_engine(P, T, Bn, fl)
    pl = run_engine(eng, batch, 0)
    for got, want, k in zip(engine_outs(eng, pl), outs, OUTS):
        e = relmax(got, want)
        log(f"gru4rec amid edge {variant} B{Bn} T{T}: {k} {e:.3e} (gate margin {margin:.2e})")
        assert e < 1e-4, (k, e)
    if fl["isDR"]:
        lc, le, _ = (float(v) for v in pl.dr_losses.cpu())
        assert abs(lc + 0.1 * le - float(loss)) < 1e-5
    else:
        assert abs(float(pl.loss.item()) - float(loss)) < 1e-5
    grads_check(f"gru4rec amid edge {variant} B{Bn} T{T}", eng, pl, grads, 5e-4, 5e-4)


@pytest.mark.parametrize("variant", ["itc", "inc_itc"])
def test_a_padded_batch_with_every_gate_off(variant):
    """Left-padded sequences and thresholds no softmax reaches: every gate is zero (asserted in float64), the modules add their biases
    only; outputs only."""
    Bn, T = 17, 20
    fl = full_flags(dict(VARIANTS[variant], threshold1=0.9, threshold2=0.9))
    shapes = ref.gru4rec_amid_param_shapes(N_EDGE, D, HID_EDGE, Bn, fl["isInC"], fl["isItC"], fl["isDR"])
    P = orc.random_params(shapes, seed=71)
    ref.scale_params(P, 0.05, 1.0)
    batch = orc.synthetic_batch(Bn, T, N_EDGE - 1, pad_id=N_EDGE - 1, neg=1, seed=72)
    taps = {}
    with torch.no_grad():
        outs = ref.gru4rec_amid_forward({k: v.double() for k, v in P.items()}, batch["i_node"], batch["neg_samples"], batch["seq_d1"],
                                        batch["seq_d2"], taps=taps, **fl)
    for mname in (["inc_d1", "inc_d2"] if fl["isInC"] else []) + ["itc_d1", "itc_d2"]:
        assert float(taps[mname]["gate"].sum()) == 0.0 and taps[mname]["margin"] > 0.1, mname
    eng = make_engine(P, T, Bn, fl)
    pl = run_engine(eng, batch, need_grad=False)
    assert float(pl.itc_gate.abs().sum()) == 0.0
    for got, want, k in zip(engine_outs(eng, pl), outs, OUTS):
        assert relmax(got, want) < 1e-4, k


# ---------------------------------------------------------------------------- 4. train steps on two Adam states
def test_five_pool_steps_track_fp64_adam_on_two_states():
    """isItC + isDR: five pool_step()s, graph replay, alternating the two objectives, each on its own Adam state and pool, against two
    float64 torch.optim.Adam instances over tests/gru_amid_ref.py: every parameter within 1e-4, the objectives within 1e-4 (the plain
    model's bars, test_five_pool_steps_track_fp64_adam)."""
    n_items, T, hid, Bn, K, lrs, w = 400, 20, 16, 24, 5, (1e-3, 5e-4), 0.1
    shapes = ref.gru4rec_amid_param_shapes(n_items, D, hid, Bn, False, True, True)
    P = orc.random_params(shapes, seed=77)
    ref.scale_params(P, 0.25, 2.0)
    g = torch.Generator().manual_seed(5)
    batches = []
    for t in range(K):
        b = orc.synthetic_batch(Bn, T, 300, pad_id=n_items - 1, neg=1, seed=900 + t)
        b["seq_d1"], b["seq_d2"] = torch.randint(1, 300, (Bn, T), generator=g), torch.randint(1, 300, (Bn, T), generator=g)
        b["ob_label"] = (torch.rand(Bn, generator=g) < 0.6).long()
        batches.append(b)
    P64 = {k: v.double() for k, v in P.items()}
    sms = []
    for b in batches:
        taps = {}
        with torch.no_grad():
            ref.gru4rec_amid_forward(P64, b["i_node"], b["neg_samples"], b["seq_d1"], b["seq_d2"], isItC=True, isDR=True, taps=taps)
        sms.append(taps["itc_d1"]["softmax"])
    ts2, _ = pick_threshold(sms)
    fl = dict(isItC=True, isDR=True, threshold2=ts2)
    m = make_model(n_items, T, hid, Bn, fl, lr=lrs[0], seed=1)
    m.load_state_dict(P, strict=True)
    eng = m.engine
    eng.dr_e_w = w
    order = [t % 2 for t in range(K)]                                       # objective (= Adam state) of step t
    for k in (0, 1):
        mine = [b for b, o in zip(batches, order) if o == k]
        ep = {key: torch.stack([b[key] for b in mine]).cuda() for key in ("i_node", "neg_samples", "seq_d1", "seq_d2", "domain_id", "ob_label")}
        ep["label"] = batches[0]["label"].cuda()
        eng.select_optimizer(k, lr=lrs[k])
        assert m.begin_epoch_pool(ep, dr_objective=k) == len(mine)
    pl = m._pool_plan
    got = []
    for k in order:
        eng.select_optimizer(k)
        out = m.pool_step(dr_objective=k)
        eng.sync()
        assert eng.has_graph(pl)
        lc, le, lr_ = (float(v) for v in out.cpu())
        got.append(lc + w * le if k == 0 else lr_)
    eng.select_optimizer(0)
    leaves = {k: v.double().clone().requires_grad_(True) for k, v in P.items()}
    opts = [torch.optim.Adam(list(leaves.values()), lr=lr) for lr in lrs]
    for t, (b, k) in enumerate(zip(batches, order)):
        opts[k].zero_grad()
        taps = {}
        outs = ref.gru4rec_amid_forward(leaves, b["i_node"], b["neg_samples"], b["seq_d1"], b["seq_d2"], taps=taps, **fl)
        assert taps["itc_d1"]["margin"] >= 1e-3 * ts2, (t, taps["itc_d1"]["margin"])
        _, _, tot, lr_ = orc.dr_losses(outs, b["label"].double(), b["domain_id"], b["ob_label"], w)
        loss = tot if k == 0 else lr_
        loss.backward()
        opts[k].step()
        assert abs(got[t] - float(loss.detach())) < 1e-4, (t, got[t], float(loss.detach()))
    sd = m.state_dict()
    worst = 0.0
    for k, v in leaves.items():
        d = float((sd[k].detach().cpu().double() - v.detach()).abs().max())
        worst = max(worst, d)
        assert d < 1e-4, (k, d)
    log(f"gru4rec amid pool steps (isItC + isDR, two Adam states): worst |param diff| to fp64 Adam after {K} steps {worst:.3e}")


def test_reference_loop_with_amid_optim_adam():
    """isItC through the reference's own loop -- forward, a loss written in torch, zero_grad / backward / step of amid_amd.optim.Adam (the
    sparse table gradient, lazy rows) -- against float64 dense Adam on the restatement, at test_reference_loop_gru4rec's bars."""
    from amid_amd.optim import Adam
    from tests.test_gpu_optim import assert_replay_exercised, bce_loss, check_params, dev, loop_batches, verbatim_step
    n_items, T, hid, Bn, lr = 200, 12, 16, 5, 1e-3
    P = orc.random_params(ref.gru4rec_amid_param_shapes(n_items, D, hid, Bn, isItC=True), seed=77)
    ref.scale_params(P, 0.25, 2.0)
    batches = loop_batches(lambda t: orc.synthetic_batch(Bn, T, 50, pad_id=n_items - 1, neg=1, seed=900 + t), 6, 60, n_items - 1)
    assert_replay_exercised(batches)
    P64 = {k: v.double() for k, v in P.items()}
    sms = []
    for b in batches:
        taps = {}
        with torch.no_grad():
            ref.gru4rec_amid_forward(P64, b["i_node"], b["neg_samples"], b["seq_d1"], b["seq_d2"], isItC=True, taps=taps)
        sms.append(taps["itc_d1"]["softmax"])
    got = pick_threshold(sms)
    assert got is not None
    fl = dict(isItC=True, threshold2=got[0])
    m = make_model(n_items, T, hid, Bn, fl, lr=lr, seed=1).cuda()
    m.load_state_dict(P, strict=True)
    m.train()
    optimizer = Adam(m.parameters(), lr=lr)
    Po = {k: v.double() for k, v in P.items()}
    opt_o = orc.DenseAdam(Po, lr=lr)
    for t, batch in enumerate(batches):
        loss, _, _ = verbatim_step(m, optimizer, dev(batch), bce_loss)
        optimizer.step()
        taps = {}
        loss_o, _, grads = ref.loss_and_grads(Po, batch, taps=taps, **fl)
        assert taps["itc_d1"]["margin"] >= 1e-3 * got[0], (t, taps["itc_d1"]["margin"])
        opt_o.step(Po, grads)
        assert abs(loss.item() - float(loss_o)) < 5e-5, t
    check_params(m, Po, tag="gru4rec isItC")


# ---------------------------------------------------------------------------- 5. evaluation
@pytest.mark.parametrize("B,T,NI", [(33, 20, 100), (7, 17, 5)])
@pytest.mark.parametrize("variant", ["itc", "inc", "inc_itc", "itc_dr", "dr"])
def test_eval_batch_is_bit_identical_to_the_forward_and_rank_kernels(variant, B, T, NI):
    """enqueue_eval gives the bits of enqueue_forward(train=False) + the rank kernel per variant: the rows of x[2] the head reads (isItC:
    every sequence; otherwise the own-domain ones), the scores, both ranks; the loss parts to 1e-6."""
    from tests.test_gpu_bert_eval import FIX, HID, N_ITEMS, eval_batch, live_rows, old_path, poison
    fl = full_flags(dict(VARIANTS.get(variant, dict(isDR=True)), threshold1=1.0 / B, threshold2=1.0 / B))
    P = orc.random_params(ref.gru4rec_amid_param_shapes(N_ITEMS, D, HID, B, fl["isInC"], fl["isItC"], fl["isDR"]), seed=3 + T)
    ref.scale_params(P, 0.25, 2.0)
    eng = make_engine(P, T, B, fl)
    pl = eng.plan(B, T, NI, need_grad=False)
    Tenc = pl.shape.Tenc
    assert eng.eval_fused_ok(pl) and Tenc == (2 * T if fl["isInC"] else T)
    rows = (lambda x, cu: x.reshape(2, B, Tenc, D)) if fl["isItC"] else (lambda x, cu: live_rows(x, cu, B, Tenc))
    for seed, dom in ((40, None), (41, 0), (42, 1)):
        cu = {k: v.cuda() for k, v in eval_batch(B, T, NI, seed, dom).items()}
        torch.cuda.synchronize()
        own, r, r0 = old_path(eng, pl, cu)
        x_old = rows(pl.x[2].clone(), cu).clone()
        gate_old = pl.itc_gate.clone() if fl["isItC"] else None
        poison(eng, pl)
        pl.gi.fill_(float("nan"))
        torch.cuda.synchronize()
        eng.load_batch(pl, *(cu[k] for k in KEYS))
        eng.enqueue_eval(pl, FIX, with_loss=True, want_scores=True)
        eng.sync()
        eng.check_index_error(pl)
        assert bool(torch.isfinite(x_old).all()) and torch.equal(rows(pl.x[2].clone(), cu), x_old)
        if gate_old is not None:
            assert torch.equal(pl.itc_gate, gate_old)
            log(f"gru4rec amid eval {variant} B{B}: {int(gate_old.sum())} of {B} gates on")
        assert torch.equal(pl.ev_p, own), float((pl.ev_p - own).abs().max())
        assert torch.equal(pl.ev_rank, r) and torch.equal(pl.ev_rank_raw, r0)
        want = torch.nn.functional.binary_cross_entropy(own.double(), cu["label"].double(), reduction="none").sum(1) / (B * NI)
        assert float((pl.ev_loss_part.double() - want).abs().max()) <= 1e-6 * float(want.abs().max()) + 1e-9


# ---------------------------------------------------------------------------- 6. serving
def test_encode_then_score_is_recommend_all_for_isitc():
    from tests.test_gpu_embeddings import own_history
    from tests.test_gpu_recommend_all import _users
    n, B, T, k = 3, 8, 20, 10
    model = make_model(120, T, 16, B, dict(isItC=True, threshold2=1.0 / B), seed=2)
    model.eval()
    users = _users(n, B, T, seed=T + 3)
    pools = (torch.arange(1, 61, dtype=torch.int64).cuda(), torch.arange(40, 102, dtype=torch.int64).cuda())
    vec = model.encode_users(users, use_graph=True)
    assert vec.shape == (n, B, D) and torch.equal(vec, model.encode_users(users, use_graph=False))
    assert bool(torch.isfinite(vec).all()) and float(vec.abs().max()) > 0
    want_i, want_s = model.recommend_all(users, k=k, pool=pools)
    hist = own_history(users)
    for i in range(n):
        got_i, got_s = model.recommend_from_vectors(vec[i], users["domain_id"][i], k=k, pool=pools, history=hist[i])
        assert torch.equal(got_i, want_i[i]) and torch.equal(got_s, want_s[i]), i
        one_i, one_s = model.recommend(users["seq_d1"][i], users["seq_d2"][i], users["domain_id"][i], k=k, pool=pools)
        assert torch.equal(one_i, want_i[i]) and torch.equal(one_s, want_s[i]), i
    with pytest.raises(ValueError):                                   # the "exactly bs rows" check
        model.encode_users({key: v[:, :5] for key, v in users.items()})


# ---------------------------------------------------------------------------- 7. checkpoint
def test_resumed_run_is_the_uninterrupted_run(tmp_path):
    """isItC + isDR, both objectives on their Adam states: k steps, save, more steps; a model of another seed loads the file and takes the
    same steps: the losses and the whole training state, bit for bit.  A checkpoint of the plain class loads into this one and back."""
    from tests.test_gpu_checkpoint import B as CB, N_ITEMS as CN, T as CT, _assert_same, _epoch, _flushed_state, _steps
    fl = dict(isItC=True, isDR=True, threshold2=1.0 / CB)
    ep = _epoch(6, seed=11, hot=(4,))

    def both(m, idx):
        out = []
        for k, lr in ((0, 1e-3), (1, 5e-4)):
            m.engine.select_optimizer(k, lr=lr)
            out += _steps(m, ep, idx, k=k)
        return out

    a = make_model(CN, CT, 16, CB, fl, lr=1e-3, seed=3)
    both(a, range(3))
    path = str(tmp_path / "state.pt")
    a.save_training_state(path, epoch=1)
    la = both(a, range(3, 6))
    b = make_model(CN, CT, 16, CB, fl, lr=1e-3, seed=4)
    assert b.load_training_state(path) == {"epoch": 1}
    lb = both(b, range(3, 6))
    assert len(la) == len(lb) == 6
    for x, y in zip(la, lb):
        assert torch.equal(x, y)
    _assert_same(_flushed_state(a), _flushed_state(b))
    # flags all off: the two classes hold the same model
    from amid_amd.model_gru import GRU4Rec
    p = GRU4Rec(10, D, CN, D, CT, 16, CB, False, False, 0.5, 0.5, lr=1e-3, seed=7)
    _steps(p, ep, range(2))
    p.save_training_state(str(tmp_path / "plain.pt"))
    q = make_model(CN, CT, 16, CB, {}, lr=1e-3, seed=8)
    q.load_training_state(str(tmp_path / "plain.pt"))
    for x, y in zip(_steps(p, ep, range(2, 4)), _steps(q, ep, range(2, 4))):
        assert torch.equal(x, y)
    q.save_training_state(str(tmp_path / "amid.pt"))
    GRU4Rec(10, D, CN, D, CT, 16, CB, False, False, 0.5, 0.5, seed=9).load_training_state(str(tmp_path / "amid.pt"))
    sp, sq = p.state_dict(), q.state_dict()
    assert list(sp) == list(sq)


# ---------------------------------------------------------------------------- 8. the command lines
def test_cli_train_sr_dr_then_recommend(tmp_path):
    """run.sh's command line with --model gru4rec on toy CSVs (as test_train_sr_dr_cli_end_to_end for SASRec): one epoch, two seeds, then
    recommend.py on the saved weights; a wrong batch size is the "exactly bs rows" error."""
    from amid_amd import recommend
    from amid_amd.train_sr_dr import main
    from tests.test_gpu_module import _write_csv
    rng = np.random.default_rng(2)
    root = tmp_path / "mybank_dataset"
    root.mkdir()
    _write_csv(root / "toy_train25.csv", 128, rng, 1, 400, 400, 900)
    _write_csv(root / "toy_train25_DR.csv", 96, rng, 1, 400, 400, 900, ob_label=True)
    _write_csv(root / "toy_test.csv", 64, rng, 1, 400, 400, 900)
    common = ["--data_root", str(tmp_path), "-ds", "mybank", "-dm", "toy", "--overlap_ratio", "0.25", "--model", "gru4rec", "--isItC", "True",
              "--ts2", "0.03", "--neg_nums", "19", "--bs", "32", "--seq_len", "20", "--emb_dim", "128", "--hid_dim", "16"]
    summary = main(common + ["--overlap", "True", "--lr2", "0.01", "--dr_e_w", "0.01", "--epoch", "1", "--seeds", "2", "-md", str(tmp_path / "model"),
                             "--save_dir", str(tmp_path / "run")])
    assert len(summary) == 2
    for best in summary:
        assert ("d1", "HR@10") in best and all((0.0 <= v <= 1.0) or np.isnan(v) for v in best.values())
    text = (tmp_path / "model" / "log1.txt").read_text()
    assert "train loss_dr_r" in text and "dr_e loss" in text
    K = 5
    res = recommend.main(common + ["--isDR", "True", "--weights", str(tmp_path / "run" / "seed0" / "best_d1.pt"), "--topk", str(K),
                                   "--out", str(tmp_path / "top.npz")])
    items = np.load(tmp_path / "top.npz")["items"]
    assert items.shape == (64, K) and bool((items >= 0).all()) and np.array_equal(res["items"], items)
    m = make_model(120, 20, 16, 32, dict(isItC=True))
    z = torch.zeros(8, dtype=torch.long, device="cuda")
    with pytest.raises(ValueError, match="exactly bs"):
        m.train_step(z, z.view(8, 1), z.view(8, 1).repeat(1, 20), z.view(8, 1).repeat(1, 20), torch.zeros(8, 2, device="cuda"), z)


# ---------------------------------------------------------------------------- 9. staying out
def test_refusals_kept():
    from amid_amd.model_gru import GRU4Rec
    with pytest.raises(ValueError, match="GRU4RecAMID"):
        GRU4Rec(10, D, 100, D, 20, 32, 4, False, True, 0.5, 0.5)
    with pytest.raises(ValueError):
        make_model(100, 20, 32, 4, dict(isItC=True), compute="bf16")
    from amid_amd.model_gru import GRU4RecAMID
    with pytest.raises(ValueError):
        GRU4RecAMID(10, 64, 100, 64, 20, 32, 4, False, True, 0.5, 0.5)

    class World2:
        world = 2
    m = make_model(100, 20, 32, 4, dict(isItC=True, isDR=True))
    z = torch.zeros(4, dtype=torch.long, device="cuda")
    with pytest.raises(NotImplementedError):
        m.train_step(z, z.view(4, 1), z.view(4, 1).repeat(1, 20), z.view(4, 1).repeat(1, 20), torch.zeros(4, 2, device="cuda"), z, exchange=World2())
