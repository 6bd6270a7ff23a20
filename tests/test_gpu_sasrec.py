"""GPU parity of the whole SASRec path (forward, loss, backward, optimizer, graph replay) against
the CPU oracle and the reference-generated golden vectors.  Everything runs through libamid_hip.so."""
import copy
import os

import numpy as np
import pytest
import torch

from oracle import amid_oracle as orc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LOG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")


def log(msg):
    os.makedirs(LOG, exist_ok=True)
    with open(os.path.join(LOG, "parity.log"), "a") as f:
        f.write(msg + "\n")


def relmax(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def make_engine(P, T, lr=5e-4, seed=0):
    from amid_amd.engine import SasrecEngine
    n_rows, D = P["item_emb_layer.emb_item.weight"].shape
    hid = P["predictModule.fc.0.weight"].shape[0]
    eng = SasrecEngine(n_rows, D, T, hid, lr=lr, seed=seed)
    eng.load_state_dict(P)
    return eng


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name))
    P = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("P/")}
    B = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("B/")}
    G = {k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("G/")}
    return z, P, B, G


def run_forward(eng, batch, train, with_loss, step=None, seed=None):
    Bn, T = batch["seq_d1"].shape
    NI = 1 + batch["neg_samples"].shape[1]
    pl = eng.plan(Bn, T, NI, need_grad=True)
    if step is not None:
        eng.set_step(step, seed)
    cu = {k: v.cuda() for k, v in batch.items()}
    eng.load_batch(pl, cu["i_node"], cu["neg_samples"], cu["seq_d1"], cu["seq_d2"], cu.get("label"), cu.get("domain_id"))
    eng.enqueue_prepare(pl, sparse=True)
    eng.enqueue_forward(pl, train=train, with_loss=with_loss)
    eng.sync()
    eng.check_index_error(pl)
    return pl


def dense_table_grad(eng, pl):
    U = int(pl.n_uniq.item())
    g = torch.zeros(eng.n_rows, eng.D)
    g[pl.uniq_ids[:U].cpu().long()] = pl.uniq_grad[:U].cpu()
    return g


def compare_taps(tag, eng, pl, P, batch, masks):
    """Stage-by-stage diagnostics against the oracle (written to gpurun_out/parity.log)."""
    taps = {}
    orc.sasrec_forward(P, batch["i_node"], batch["neg_samples"], batch["seq_d1"], batch["seq_d2"], masks, taps)
    Bn, T = batch["seq_d1"].shape
    M, D = Bn * T, eng.D
    for g, s in enumerate(("sac1", "sac2")):
        for i in range(3):
            got = pl.x[i][g * M:(g + 1) * M].reshape(Bn, T, D)
            log(f"{tag} {s} x{i}: relmax {relmax(got, taps[s][f'x{i}']):.3e}")
    log(f"{tag} u1 {relmax(pl.u[0], taps['u1']):.3e} u2 {relmax(pl.u[1], taps['u2']):.3e}")


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("train", [False, True])
def test_forward_logits_vs_oracle(D, train):
    T, Bn, hid, n_items = 50, 9, 32, 500
    P = orc.random_params(orc.sasrec_param_shapes(n_items, D, T, hid), seed=D)
    batch = orc.synthetic_batch(Bn, T, n_items - 1, pad_id=n_items - 1, neg=1, seed=3)
    eng = make_engine(P, T, seed=77)
    masks = orc.philox_masks_sasrec(Bn, T, D, seed=77, step=5) if train else None
    pl = run_forward(eng, batch, train=train, with_loss=False, step=5, seed=77)
    compare_taps(f"fwd D={D} train={train}", eng, pl, P, batch, masks)
    p1, p2 = orc.sasrec_forward(P, batch["i_node"], batch["neg_samples"], batch["seq_d1"], batch["seq_d2"], masks)
    e1, e2 = relmax(pl.p1, p1), relmax(pl.p2, p2)
    log(f"fwd D={D} train={train}: logits relmax {e1:.3e} {e2:.3e}")
    assert e1 < 1e-4 and e2 < 1e-4          # north-star tolerance on fp32 logits
    assert e1 < 2e-5 and e2 < 2e-5          # what the kernels actually deliver


def test_forward_golden_sasrec_eval():
    for name in ("g3_sasrec_eval.npz", "g3_sasrec_eval_neg9.npz"):
        z, P, B, _ = load_golden(name)
        eng = make_engine(P, 50)
        pl = run_forward(eng, B, train=False, with_loss=False)
        assert relmax(pl.p1, z["p1"]) < 1e-4 and relmax(pl.p2, z["p2"]) < 1e-4
        log(f"golden {name}: {relmax(pl.p1, z['p1']):.3e} {relmax(pl.p2, z['p2']):.3e}")


def test_encoder_golden_log2feats_d128():
    """Log2feats forward straight from the reference (g2): feed its input rows through the table."""
    z = np.load(os.path.join(GOLDEN, "g2_log2feats_d128.npz"))
    x, y = torch.from_numpy(z["x"]), torch.from_numpy(z["y"])
    Bn, T, D = x.shape
    P = orc.random_params(orc.sasrec_param_shapes(Bn * T + 4, D, T, 16), seed=1)
    for k in z.files:
        if k.startswith("P/sac1."):
            P[k[2:]] = torch.from_numpy(z[k])
            P[k[2:].replace("sac1.", "sac2.")] = torch.from_numpy(z[k])
    P["item_emb_layer.emb_item.weight"][: Bn * T] = x.reshape(Bn * T, D)
    seq = torch.arange(Bn * T).reshape(Bn, T)
    batch = dict(i_node=torch.zeros(Bn, dtype=torch.long), neg_samples=torch.ones(Bn, 1, dtype=torch.long), seq_d1=seq, seq_d2=seq)
    eng = make_engine(P, T)
    pl = run_forward(eng, batch, train=False, with_loss=False)
    want_u = y.mean(1)
    assert relmax(pl.u[0], want_u) < 1e-5 and relmax(pl.u[1], want_u) < 1e-5


def grads_check(tag, eng, pl, grads, tol, l2tol):
    worst = 0.0
    for name in eng.dense.slots:
        got = eng.dense.view(name, eng.dense.grad)
        e, e2 = relmax(got, grads[name]), rel_l2(got, grads[name])
        if name.endswith("in_proj_bias"):            # the key-bias third is analytically zero
            D = got.numel() // 3
            gg, ww = got.cpu().clone(), grads[name].clone()
            gg[D:2 * D] = 0; ww[D:2 * D] = 0
            e, e2 = relmax(gg, ww), rel_l2(gg, ww)
        log(f"{tag} grad {name:50s} relmax {e:.3e} l2 {e2:.3e}")
        worst = max(worst, e)
        assert e < tol and e2 < l2tol, (name, e, e2)
    tg = dense_table_grad(eng, pl)
    e, e2 = relmax(tg, grads["item_emb_layer.emb_item.weight"]), rel_l2(tg, grads["item_emb_layer.emb_item.weight"])
    log(f"{tag} grad table relmax {e:.3e} l2 {e2:.3e}; worst dense {worst:.3e}")
    assert e < tol and e2 < l2tol


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("train", [False, True])
def test_backward_grads_vs_oracle(D, train):
    T, Bn, hid, n_items = 50, 7, 32, 400
    P = orc.random_params(orc.sasrec_param_shapes(n_items, D, T, hid), seed=10 + D)
    batch = orc.synthetic_batch(Bn, T, n_items - 1, pad_id=n_items - 1, neg=1, seed=4)
    seed, step = 99, 2
    masks = orc.philox_masks_sasrec(Bn, T, D, seed=seed, step=step) if train else None
    taps = {}
    orc.sasrec_forward({k: v.double() for k, v in P.items()}, batch["i_node"], batch["neg_samples"], batch["seq_d1"], batch["seq_d2"],
                       None if masks is None else {k: v.double() for k, v in masks.items()}, taps)
    margin = min(taps[s][f"relu_margin{l}"] for s in ("sac1", "sac2") for l in (0, 1))
    log(f"bwd D={D} train={train}: relu margin {margin:.3e}")
    loss, (p1, p2), grads = orc.loss_and_grads("sasrec", P, batch, masks)
    eng = make_engine(P, T, seed=seed)
    pl = run_forward(eng, batch, train=train, with_loss=True, step=step, seed=seed)
    eng.enqueue_backward(pl, train=train)
    eng.sync()
    assert abs(float(pl.loss.item()) - float(loss)) < 1e-5 * max(1.0, abs(float(loss)))
    assert relmax(pl.p1, p1) < 2e-5
    # max-abs comparison is only meaningful when no relu pre-activation sits on the kink
    tol = 2e-4 if margin > 2e-5 else 5e-2
    grads_check(f"bwd D={D} train={train}", eng, pl, grads, tol, 2e-4 if margin > 2e-5 else 1e-2)


def test_backward_golden_sasrec_grads():
    z, P, B, G = load_golden("g4_sasrec_grads.npz")
    B = dict(B)
    B["label"] = torch.from_numpy(z["labels"])
    eng = make_engine(P, 50)
    pl = run_forward(eng, B, train=False, with_loss=True)
    eng.enqueue_backward(pl, train=False)
    eng.sync()
    assert abs(float(pl.loss.item()) - float(z["loss"])) < 1e-5
    grads_check("golden g4", eng, pl, G, 5e-4, 5e-4)


@pytest.mark.parametrize("D", [64, 128])
def test_train_steps_track_dense_adam_reference(D):
    """K full steps (dropout on, lazy table Adam) against the oracle's dense-Adam trajectory."""
    T, Bn, hid, n_items, K = 20, 16, 32, 300, 6
    P = orc.random_params(orc.sasrec_param_shapes(n_items, D, T, hid), seed=20 + D)
    seed = 4242
    eng = make_engine(P, T, lr=1e-3, seed=seed)
    Po = {k: v.clone() for k, v in P.items()}
    opt = orc.DenseAdam(Po, lr=1e-3)
    pl = eng.plan(Bn, T, 2, need_grad=True)
    for t in range(1, K + 1):
        # items 1..60 only at steps 1,2 and 5: rows idle in between must still move (dense-Adam equivalence)
        lo_hi = (1, 60) if t in (1, 2, 5) else (100, n_items - 1)
        batch = orc.synthetic_batch(Bn, T, lo_hi[1], pad_id=n_items - 1, neg=1, seed=100 + t)
        for k in ("i_node", "neg_samples", "seq_d1", "seq_d2"):
            batch[k] = torch.where(batch[k] == n_items - 1, batch[k], batch[k].clamp(min=lo_hi[0]))
        masks = orc.philox_masks_sasrec(Bn, T, D, seed=seed, step=t)
        loss_o = orc.train_step("sasrec", Po, opt, batch, masks)
        cu = {k: v.cuda() for k, v in batch.items()}
        eng.load_batch(pl, cu["i_node"], cu["neg_samples"], cu["seq_d1"], cu["seq_d2"], cu["label"], cu["domain_id"])
        eng.enqueue_train_step(pl)
        eng.sync()
        assert eng.step == t
        log(f"traj D={D} step {t}: loss gpu {float(pl.loss.item()):.7f} oracle {loss_o:.7f}")
        assert abs(float(pl.loss.item()) - loss_o) < 5e-5
    eng.flush_table()
    eng.sync()
    sd = eng.state_dict()
    for k, v in Po.items():
        d = (sd[k].cpu() - v).abs()
        if k.endswith("in_proj_bias"):
            Dd = v.numel() // 3
            d = torch.cat((d[:Dd], d[2 * Dd:]))      # chaotic key-bias slice, see test_oracle_golden
        log(f"traj D={D} param {k:50s} maxabs {float(d.max()):.3e}")
        assert float(d.max()) < 2e-4, k


def test_graph_replay_equals_eager():
    D, T, Bn, hid, n_items = 64, 20, 8, 16, 200
    P = orc.random_params(orc.sasrec_param_shapes(n_items, D, T, hid), seed=5)
    batches = [orc.synthetic_batch(Bn, T, n_items - 1, pad_id=n_items - 1, neg=1, seed=200 + t) for t in range(4)]

    def run(use_graph):
        eng = make_engine(P, T, lr=1e-3, seed=9)
        pl = eng.plan(Bn, T, 2, need_grad=True)
        losses = []
        if use_graph:
            cu = {k: v.cuda() for k, v in batches[0].items()}
            eng.load_batch(pl, cu["i_node"], cu["neg_samples"], cu["seq_d1"], cu["seq_d2"], cu["label"], cu["domain_id"])
            eng.capture_train_step(pl)
        for b in batches:
            cu = {k: v.cuda() for k, v in b.items()}
            eng.load_batch(pl, cu["i_node"], cu["neg_samples"], cu["seq_d1"], cu["seq_d2"], cu["label"], cu["domain_id"])
            if use_graph:
                eng.replay_train_step(pl)
            else:
                eng.enqueue_train_step(pl)
            eng.sync()
            losses.append(float(pl.loss.item()))
        eng.flush_table()
        eng.sync()
        return losses, {k: v.cpu().clone() for k, v in eng.state_dict().items()}

    l0, s0 = run(False)
    l1, s1 = run(True)
    assert l0 == l1
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k


@pytest.mark.parametrize("use_graph", [False, True])
def test_input_pool_equals_per_step_load(use_graph):
    """set_input_pool(): the step's first kernel picks its batch from the HBM-resident pool by the device step counter (wrapping
    around the pool, and starting from the step the pool was installed at); results are bit-identical to copying each batch in."""
    D, T, Bn, hid, n_items = 64, 20, 8, 16, 200
    P = orc.random_params(orc.sasrec_param_shapes(n_items, D, T, hid), seed=5)
    batches = [orc.synthetic_batch(Bn, T, n_items - 1, pad_id=n_items - 1, neg=1, seed=300 + t) for t in range(3)]
    n_steps, pre_steps = 7, 2

    def run(pool_mode):
        eng = make_engine(P, T, lr=1e-3, seed=9)
        pl = eng.plan(Bn, T, 2, need_grad=True)
        packed = []
        for b in batches:
            cu = {k: v.cuda() for k, v in b.items()}
            packed.append(eng.pack_batch(pl, cu["i_node"], cu["neg_samples"], cu["seq_d1"], cu["seq_d2"], cu["label"], cu["domain_id"]))
        for t in range(pre_steps):                       # the pool is installed at a non-zero step
            eng.load_packed(pl, packed[2 - t])
            eng.enqueue_train_step(pl)
        if pool_mode:
            eng.set_input_pool(pl, torch.stack(packed))
        else:
            eng.load_packed(pl, packed[0])
        if use_graph:
            eng.capture_train_step(pl)
        losses = []
        for t in range(n_steps):
            if not pool_mode:
                eng.load_packed(pl, packed[t % 3])
            if use_graph:
                eng.replay_train_step(pl)
            else:
                eng.enqueue_train_step(pl)
            eng.sync()
            losses.append(float(pl.loss.item()))
            if pool_mode:
                assert torch.equal(pl.in_pack, packed[t % 3])      # the image is mirrored into the static input words
        eng.check_index_error(pl)
        eng.flush_table()
        eng.sync()
        return losses, {k: v.cpu().clone() for k, v in eng.state_dict().items()}

    l0, s0 = run(False)
    l1, s1 = run(True)
    assert l0 == l1
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k


def test_input_pool_rejects_wrong_layout():
    D, T, Bn, hid, n_items = 64, 20, 8, 16, 200
    P = orc.random_params(orc.sasrec_param_shapes(n_items, D, T, hid), seed=5)
    eng = make_engine(P, T)
    pl = eng.plan(Bn, T, 2, need_grad=True)
    with pytest.raises(ValueError):
        eng.set_input_pool(pl, torch.zeros(4, pl.in_words + 1, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        eng.set_input_pool(pl, torch.zeros(4, pl.in_words, dtype=torch.int32, device="cuda"))
    eng.set_input_pool(pl, torch.zeros(4, pl.in_words, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        eng.enqueue_prepare(pl, sparse=True)             # a pool only advances with the step
    eng.set_input_pool(pl, None)
    eng.enqueue_prepare(pl, sparse=True)
    eng.sync()


# ---------------------------------------------------------------------------- isItC (next-1 of SURVEY.md section 8(f))
def make_itc_engine(P, T, bs, ts2, lr=5e-4, seed=0):
    from amid_amd.engine import SasrecEngine
    n_rows, D = P["item_emb_layer.emb_item.weight"].shape
    hid = P["predictModule.fc.0.weight"].shape[0]
    eng = SasrecEngine(n_rows, D, T, hid, lr=lr, seed=seed, itc_bs=bs, itc_threshold=ts2)
    eng.load_state_dict(P)
    return eng


def test_itc_golden_logits_loss_grads():
    """SASRec(isItC=True) against the reference's own logits, loss and gradients (g10; trans_nn / trans_bs included)."""
    z, P, B, G = load_golden("g10_sasrec_itc.npz")
    B = dict(B)
    B["label"] = torch.from_numpy(z["labels"])
    eng = make_itc_engine(P, B["seq_d1"].shape[1], B["seq_d1"].shape[0], float(z["threshold2"]))
    pl = run_forward(eng, B, train=False, with_loss=True)
    assert np.array_equal(pl.itc_gate.cpu().numpy() > 0.5, z["gate"])
    assert relmax(pl.p1, z["p1"]) < 1e-4 and relmax(pl.p2, z["p2"]) < 1e-4
    eng.enqueue_backward(pl, train=False)
    eng.sync()
    assert abs(float(pl.loss.item()) - float(z["loss"])) < 1e-5
    grads_check("golden g10 itc", eng, pl, G, 5e-4, 5e-4)


@pytest.mark.parametrize("D,train", [(64, False), (128, True)])
def test_itc_vs_oracle_and_train_steps(D, train):
    """isItC forward / backward against the oracle on unpadded rows (a non-trivial gate), then full train steps with graph replay."""
    T, Bn, hid, n_items, ts2 = 20, 8, 16, 300, 0.15
    P = orc.random_params(orc.sasrec_param_shapes(n_items, D, T, hid, itc_bs=Bn), seed=40 + D)
    for d in (1, 2):
        P[f"sac{d}.last_layernorm.weight"] *= 0.3          # keeps the batch softmax of the pair-max scores away from one-hot
    g = torch.Generator().manual_seed(7)
    batch = orc.synthetic_batch(Bn, T, n_items - 1, pad_id=n_items - 1, neg=1, seed=9)
    batch["seq_d1"] = torch.randint(1, n_items - 1, (Bn, T), generator=g)      # no shared pad positions: distinct pair-max scores
    batch["seq_d2"] = torch.randint(1, n_items - 1, (Bn, T), generator=g)
    seed, step = 31, 3
    masks = orc.philox_masks_sasrec(Bn, T, D, seed=seed, step=step) if train else None
    taps = {}
    orc.sasrec_forward(P, batch["i_node"], batch["neg_samples"], batch["seq_d1"], batch["seq_d2"], masks, taps, isItC=True, threshold2=ts2)
    gate = taps["itc_d1"]["gate"]
    log(f"itc D={D} train={train}: gate {gate.int().tolist()} softmax margin {taps['itc_d1']['margin']:.3e}")
    assert 0 < int(gate.sum()) < Bn and taps["itc_d1"]["margin"] > 1e-3
    loss, (p1, p2), grads = orc.loss_and_grads("sasrec", P, batch, masks, isItC=True, threshold2=ts2)
    eng = make_itc_engine(P, T, Bn, ts2, lr=1e-3, seed=seed)
    pl = run_forward(eng, batch, train=train, with_loss=True, step=step, seed=seed)
    assert torch.equal(pl.itc_gate.cpu(), gate)
    assert relmax(pl.p1, p1) < 3e-5 and relmax(pl.p2, p2) < 3e-5
    eng.enqueue_backward(pl, train=train)
    eng.sync()
    assert abs(float(pl.loss.item()) - float(loss)) < 1e-5
    grads_check(f"itc D={D} train={train}", eng, pl, grads, 5e-4 if train else 2e-4, 5e-3 if train else 2e-4)
    # train steps: eager vs hipGraph replay, bit-identical, and a wrong batch size is refused
    def run(use_graph):
        e = make_itc_engine(P, T, Bn, ts2, lr=1e-3, seed=seed)
        q = e.plan(Bn, T, 2, need_grad=True)
        cu = {k: v.cuda() for k, v in batch.items()}
        e.load_batch(q, cu["i_node"], cu["neg_samples"], cu["seq_d1"], cu["seq_d2"], cu["label"], cu["domain_id"])
        if use_graph:
            e.capture_train_step(q)
        losses = []
        for _ in range(3):
            e.replay_train_step(q) if use_graph else e.enqueue_train_step(q)
            e.sync()
            losses.append(float(q.loss.item()))
        e.flush_table(); e.sync()
        return losses, {k: v.cpu().clone() for k, v in e.state_dict().items()}
    l0, s0 = run(False)
    l1, s1 = run(True)
    assert l0 == l1 and all(torch.equal(s0[k], s1[k]) for k in s0)
    assert l0[2] < l0[0]
    with pytest.raises(ValueError):
        eng.plan(Bn + 1, T, 2, need_grad=True)


# ---------------------------------------------------------------------------- isInC (next-1 of SURVEY.md section 8(f))
def make_inc_engine(P, T, bs, ts1, lr=5e-4, seed=0, **kw):
    from amid_amd.engine import SasrecEngine
    n_rows, D = P["item_emb_layer.emb_item.weight"].shape
    hid = P["predictModule.fc.0.weight"].shape[0]
    eng = SasrecEngine(n_rows, D, T, hid, lr=lr, seed=seed, inc_bs=bs, inc_threshold=ts1, **kw)
    eng.load_state_dict(P)
    return eng


def test_inc_golden_logits_loss_grads():
    """SASRec(isInC=True) against the reference's own logits, loss and gradients (g12; inc_d*.trans_nn / trans_bs and the 2T-row
    pos_emb included)."""
    z, P, B, G = load_golden("g12_sasrec_inc.npz")
    B = dict(B)
    B["label"] = torch.from_numpy(z["labels"])
    T = B["seq_d1"].shape[1]
    assert P["sac1.pos_emb.weight"].shape[0] == 2 * T
    eng = make_inc_engine(P, T, B["seq_d1"].shape[0], float(z["threshold1"]))
    pl = run_forward(eng, B, train=False, with_loss=True)
    assert np.array_equal(pl.inc_gate[0].cpu().numpy() > 0.5, z["gate_d1"])
    assert np.array_equal(pl.inc_gate[1].cpu().numpy() > 0.5, z["gate_d2"])
    assert relmax(pl.p1, z["p1"]) < 1e-4 and relmax(pl.p2, z["p2"]) < 1e-4
    eng.enqueue_backward(pl, train=False)
    eng.sync()
    assert abs(float(pl.loss.item()) - float(z["loss"])) < 1e-5
    grads_check("golden g12 inc", eng, pl, G, 5e-4, 5e-4)


@pytest.mark.parametrize("D,T,train", [(64, 20, False), (128, 50, True), (128, 30, True)])
def test_inc_vs_oracle_and_train_steps(D, T, train):
    """isInC forward / backward against the oracle (2T = 40 / 60: matrix-core attention; 2T = 100: the general kernels), train-mode
    dropout over the 2T-token rows from the same counters, then full train steps with graph replay."""
    Bn, hid, n_items, ts1 = 8, 16, 300, 0.13
    P = orc.random_params(orc.sasrec_param_shapes(n_items, D, T, hid, inc_bs=Bn), seed=50 + D + T)
    P["item_emb_layer.emb_item.weight"] *= 3.0 if D == 64 else 2.2        # self pair-max scores a few units apart, softmax not flat
    g = torch.Generator().manual_seed(11)
    batch = orc.synthetic_batch(Bn, T, n_items - 1, pad_id=n_items - 1, neg=1, seed=9)
    batch["seq_d1"] = torch.randint(1, n_items - 1, (Bn, T), generator=g)
    batch["seq_d2"] = torch.randint(1, n_items - 1, (Bn, T), generator=g)
    seed, step = 33, 3
    masks = orc.philox_masks_sasrec(Bn, 2 * T, D, seed=seed, step=step) if train else None
    taps = {}
    orc.sasrec_forward(P, batch["i_node"], batch["neg_samples"], batch["seq_d1"], batch["seq_d2"], masks, taps, isInC=True, threshold1=ts1)
    for d in (1, 2):
        gate = taps[f"inc_d{d}"]["gate"]
        log(f"inc D={D} T={T} train={train} d{d}: gate {gate.int().tolist()} softmax margin {taps[f'inc_d{d}']['margin']:.3e}")
        assert 0 < int(gate.sum()) < Bn and taps[f"inc_d{d}"]["margin"] > 1e-3
    loss, (p1, p2), grads = orc.loss_and_grads("sasrec", P, batch, masks, isInC=True, threshold1=ts1)
    eng = make_inc_engine(P, T, Bn, ts1, lr=1e-3, seed=seed)
    pl = run_forward(eng, batch, train=train, with_loss=True, step=step, seed=seed)
    for d in (1, 2):
        assert torch.equal(pl.inc_gate[d - 1].cpu(), taps[f"inc_d{d}"]["gate"])
    assert relmax(pl.p1, p1) < 3e-5 and relmax(pl.p2, p2) < 3e-5
    eng.enqueue_backward(pl, train=train)
    eng.sync()
    assert abs(float(pl.loss.item()) - float(loss)) < 1e-5
    grads_check(f"inc D={D} T={T} train={train}", eng, pl, grads, 5e-4 if train else 2e-4, 5e-3 if train else 2e-4)

    def run(use_graph):
        e = make_inc_engine(P, T, Bn, ts1, lr=1e-3, seed=seed)
        q = e.plan(Bn, T, 2, need_grad=True)
        cu = {k: v.cuda() for k, v in batch.items()}
        e.load_batch(q, cu["i_node"], cu["neg_samples"], cu["seq_d1"], cu["seq_d2"], cu["label"], cu["domain_id"])
        if use_graph:
            e.capture_train_step(q)
        losses = []
        for _ in range(3):
            e.replay_train_step(q) if use_graph else e.enqueue_train_step(q)
            e.sync()
            losses.append(float(q.loss.item()))
        e.flush_table(); e.sync()
        return losses, {k: v.cpu().clone() for k, v in e.state_dict().items()}
    l0, s0 = run(False)
    l1, s1 = run(True)
    assert l0 == l1 and all(torch.equal(s0[k], s1[k]) for k in s0)
    assert l0[2] < l0[0]
    with pytest.raises(ValueError):
        eng.plan(Bn + 1, T, 2, need_grad=True)


@pytest.mark.parametrize("dr", [False, True])
def test_inc_plus_itc_vs_oracle(dr):
    """isInC and isItC together (InnerComp before the encoders, InterComp after them over the 2T-token features), optionally with the
    doubly-robust heads: outputs, loss and every gradient against the oracle."""
    from amid_amd.engine import SasrecEngine
    D, T, Bn, hid, n_items, ts1, ts2 = 64, 20, 8, 16, 300, 0.13, 0.15
    P = orc.random_params(orc.sasrec_param_shapes(n_items, D, T, hid, itc_bs=Bn, inc_bs=Bn, dr=dr), seed=61)
    P["item_emb_layer.emb_item.weight"] *= 3.0
    for d in (1, 2):
        P[f"sac{d}.last_layernorm.weight"] *= 0.3
    g = torch.Generator().manual_seed(13)
    batch = orc.synthetic_batch(Bn, T, n_items - 1, pad_id=n_items - 1, neg=1, seed=9)
    batch["seq_d1"] = torch.randint(1, n_items - 1, (Bn, T), generator=g)
    batch["seq_d2"] = torch.randint(1, n_items - 1, (Bn, T), generator=g)
    kw = dict(isInC=True, threshold1=ts1, isItC=True, threshold2=ts2)
    taps = {}
    orc.sasrec_forward(P, batch["i_node"], batch["neg_samples"], batch["seq_d1"], batch["seq_d2"], None, taps, isDR=dr, **kw)
    for pre in ("inc_d1", "inc_d2", "itc_d1"):
        log(f"inc+itc dr={dr} {pre}: gate {taps[pre]['gate'].int().tolist()} margin {taps[pre]['margin']:.3e}")
        assert taps[pre]["margin"] > 1e-3
    assert 0 < int(taps["itc_d1"]["gate"].sum()) < Bn
    eng = SasrecEngine(n_items, D, T, hid, lr=1e-3, seed=1, itc_bs=Bn, itc_threshold=ts2, inc_bs=Bn, inc_threshold=ts1, dr=dr)
    eng.load_state_dict(P)
    if dr:
        batch["ob_label"] = torch.tensor([1, 0, 1, 1, 0, 1, 0, 1])
        info, outs, grads = orc.dr_loss_and_grads(P, batch, "e", dr_e_w=0.1, **kw)
        pl = eng.plan(Bn, T, 2, need_grad=True)
        cu = {k: v.cuda() for k, v in batch.items()}
        eng.load_batch(pl, cu["i_node"], cu["neg_samples"], cu["seq_d1"], cu["seq_d2"], cu["label"], cu["domain_id"], cu["ob_label"])
        eng.dr_mode = 0
        eng.enqueue_prepare(pl, sparse=True)
        eng.enqueue_forward(pl, train=False, with_loss=True)
        eng.enqueue_backward(pl, train=False)
        eng.sync()
        for got, want in zip((pl.p1, pl.p2, pl.ips1, pl.ips2, pl.g1, pl.g2), outs):
            assert relmax(got, want) < 3e-5
        dr_grads_check("inc+itc+dr", eng, pl, grads, 5e-4)
        tg = dense_table_grad(eng, pl)
        assert relmax(tg, grads["item_emb_layer.emb_item.weight"]) < 5e-4
        return
    loss, (p1, p2), grads = orc.loss_and_grads("sasrec", P, batch, None, **kw)
    pl = run_forward(eng, batch, train=False, with_loss=True)
    assert torch.equal(pl.itc_gate.cpu(), taps["itc_d1"]["gate"])
    assert relmax(pl.p1, p1) < 3e-5 and relmax(pl.p2, p2) < 3e-5
    eng.enqueue_backward(pl, train=False)
    eng.sync()
    assert abs(float(pl.loss.item()) - float(loss)) < 1e-5
    grads_check("inc+itc", eng, pl, grads, 2e-4, 2e-4)


@pytest.mark.parametrize("variant", ["itc", "inc"])
def test_comp_modules_at_seq_len_150(variant):
    """The reference's amazon sequence length (train_sr_dr.py:550: 150) with InterComp (pair-max over 150 x 150 pairs, both domains'
    rows of a batch row in LDS) and with InnerComp (encoders over 300 tokens): logits, loss and gradients against the oracle."""
    from amid_amd.engine import SasrecEngine
    D, T, Bn, hid, n_items = 128, 150, 4, 16, 400
    kw_shapes = dict(itc_bs=Bn) if variant == "itc" else dict(inc_bs=Bn)
    P = orc.random_params(orc.sasrec_param_shapes(n_items, D, T, hid, **kw_shapes), seed=150)
    if variant == "itc":
        for d in (1, 2):
            P[f"sac{d}.last_layernorm.weight"] *= 0.3
    else:
        P["item_emb_layer.emb_item.weight"] *= 2.2
    g = torch.Generator().manual_seed(15)
    batch = orc.synthetic_batch(Bn, T, n_items - 1, pad_id=n_items - 1, neg=1, seed=5)
    batch["seq_d1"] = torch.randint(1, n_items - 1, (Bn, T), generator=g)
    batch["seq_d2"] = torch.randint(1, n_items - 1, (Bn, T), generator=g)
    kw = dict(isItC=True, threshold2=0.2) if variant == "itc" else dict(isInC=True, threshold1=0.2)
    taps = {}
    orc.sasrec_forward(P, batch["i_node"], batch["neg_samples"], batch["seq_d1"], batch["seq_d2"], None, taps, **kw)
    pre = "itc_d1" if variant == "itc" else "inc_d1"
    log(f"T=150 {variant}: gate {taps[pre]['gate'].int().tolist()} margin {taps[pre]['margin']:.3e}")
    assert taps[pre]["margin"] > 1e-3
    loss, (p1, p2), grads = orc.loss_and_grads("sasrec", P, batch, None, **kw)
    ekw = dict(itc_bs=Bn, itc_threshold=0.2) if variant == "itc" else dict(inc_bs=Bn, inc_threshold=0.2)
    eng = SasrecEngine(n_items, D, T, hid, lr=1e-3, seed=1, **ekw)
    eng.load_state_dict(P)
    pl = run_forward(eng, batch, train=False, with_loss=True)
    assert relmax(pl.p1, p1) < 3e-5 and relmax(pl.p2, p2) < 3e-5
    eng.enqueue_backward(pl, train=False)
    eng.sync()
    assert abs(float(pl.loss.item()) - float(loss)) < 1e-5
    grads_check(f"T=150 {variant}", eng, pl, grads, 5e-4, 5e-4)


def test_inc_train_step_vs_oracle_dense_adam():
    """Three isInC train steps (dropout on) against the oracle's dense Adam: parameters after the steps, InnerComp's included."""
    D, T, Bn, hid, n_items, ts1 = 64, 20, 8, 16, 300, 0.13
    P = orc.random_params(orc.sasrec_param_shapes(n_items, D, T, hid, inc_bs=Bn), seed=77)
    P["item_emb_layer.emb_item.weight"] *= 3.0
    g = torch.Generator().manual_seed(12)
    batch = orc.synthetic_batch(Bn, T, n_items - 1, pad_id=n_items - 1, neg=1, seed=19)
    batch["seq_d1"] = torch.randint(1, n_items - 1, (Bn, T), generator=g)
    batch["seq_d2"] = torch.randint(1, n_items - 1, (Bn, T), generator=g)
    seed, lr = 5, 1e-3
    Pref = {k: v.clone() for k, v in P.items()}
    opt = orc.DenseAdam(Pref, lr=lr)
    ref_losses = []
    for t in range(1, 4):
        masks = orc.philox_masks_sasrec(Bn, 2 * T, D, seed=seed, step=t)
        ref_losses.append(orc.train_step("sasrec", Pref, opt, batch, masks, isInC=True, threshold1=ts1))
    eng = make_inc_engine(P, T, Bn, ts1, lr=lr, seed=seed)
    pl = eng.plan(Bn, T, 2, need_grad=True)
    cu = {k: v.cuda() for k, v in batch.items()}
    eng.load_batch(pl, cu["i_node"], cu["neg_samples"], cu["seq_d1"], cu["seq_d2"], cu["label"], cu["domain_id"])
    losses = []
    for _ in range(3):
        eng.enqueue_train_step(pl)
        eng.sync()
        losses.append(float(pl.loss.item()))
    eng.flush_table(); eng.sync()
    for a, b in zip(losses, ref_losses):
        assert abs(a - float(b)) < 2e-5
    sd = eng.state_dict()
    for k, v in Pref.items():
        d = (sd[k].cpu() - v).abs()
        if k.endswith("in_proj_bias"):
            Dd = v.numel() // 3
            d = torch.cat((d[:Dd], d[2 * Dd:]))      # chaotic key-bias slice, see test_oracle_golden
        assert float(d.max()) < 2e-4, (k, float(d.max()))


# ---------------------------------------------------------------------------- isDR (next-4 of SURVEY.md section 8(f))
def dr_grads_check(tag, eng, pl, grads, tol):
    bad = []
    for name in eng.dense.slots:
        got = eng.dense.view(name, eng.dense.grad)
        want = grads[name]
        if name.endswith("in_proj_bias"):
            Dd = got.numel() // 3
            got, want = got.cpu().clone(), want.clone()
            got[Dd:2 * Dd] = 0; want[Dd:2 * Dd] = 0
        e = relmax(got, want) if float(want.abs().max()) > 1e-12 else float(torch.as_tensor(got).abs().max().cpu())
        log(f"{tag} grad {name:50s} relmax {e:.3e}")
        if not e < tol:
            bad.append((name, e))
    assert not bad, bad
    tg = dense_table_grad(eng, pl)
    assert relmax(tg, grads["item_emb_layer.emb_item.weight"]) < tol


@pytest.mark.parametrize("mode", [0, 1])
def test_dr_golden_outputs_losses_grads(mode):
    """SASRec(isDR=True, isItC=True) against the reference: six outputs, the three losses, gradients of objective `mode` (g11)."""
    from amid_amd.engine import SasrecEngine
    z, P, B, _ = load_golden("g11_sasrec_dr.npz")
    B = dict(B)
    Bn, T = B["seq_d1"].shape
    eng = SasrecEngine(P["item_emb_layer.emb_item.weight"].shape[0], 64, T, 16, itc_bs=Bn, itc_threshold=float(z["threshold2"]), dr=True,
                       dr_e_w=float(z["dr_e_w"]))
    eng.load_state_dict(P)
    eng.dr_mode = mode
    pl = eng.plan(Bn, T, 2, need_grad=True)
    cu = {k: v.cuda() for k, v in B.items()}
    eng.load_batch(pl, cu["i_node"], cu["neg_samples"], cu["seq_d1"], cu["seq_d2"], torch.from_numpy(z["labels"]).cuda(), cu["domain_id"],
                   torch.from_numpy(z["ob_label"]).cuda())
    eng.enqueue_prepare(pl, sparse=True)
    eng.enqueue_forward(pl, train=False, with_loss=True)
    eng.enqueue_backward(pl, train=False)
    eng.sync()
    for got, name in ((pl.p1, "p1"), (pl.p2, "p2"), (pl.ips1, "ips1"), (pl.ips2, "ips2"), (pl.g1, "g1"), (pl.g2, "g2")):
        assert relmax(got, z[name]) < 1e-4, name
    lc, le, lr_ = (float(v) for v in pl.dr_losses.cpu())
    assert abs(lc - float(z["loss_cls"])) < 1e-5 and abs(le - float(z["loss_dr_e"])) < 1e-5 and abs(lr_ - float(z["loss_dr_r"])) < 1e-5
    pre = "GE/" if mode == 0 else "GR/"
    G = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(pre)}
    dr_grads_check(f"golden g11 dr mode {mode}", eng, pl, G, 1e-3)


def test_dr_two_optimizers_track_oracle():
    """The doubly-robust epoch: steps of objective 0 under Adam(lr), then steps of objective 1 under a second Adam(lr * lr2) with its
    own moments (train_sr_dr.py:668-669), dropout on, lazy table rows, graph replay -- against two DenseAdam instances in the oracle."""
    from amid_amd.engine import SasrecEngine
    D, T, Bn, hid, n_items, ts2, w, lr, lr2 = 64, 20, 8, 16, 300, 0.15, 0.1, 1e-3, 0.5
    P = orc.random_params(orc.sasrec_param_shapes(n_items, D, T, hid, itc_bs=Bn, dr=True), seed=77)
    for d in (1, 2):
        P[f"sac{d}.last_layernorm.weight"] *= 0.3
    seed = 5
    eng = SasrecEngine(n_items, D, T, hid, lr=lr, seed=seed, itc_bs=Bn, itc_threshold=ts2, dr=True, dr_e_w=w)
    eng.load_state_dict(P)
    Po = {k: v.clone() for k, v in P.items()}
    opts = [orc.DenseAdam(Po, lr=lr), orc.DenseAdam(Po, lr=lr * lr2)]
    pl = eng.plan(Bn, T, 2, need_grad=True)
    g = torch.Generator().manual_seed(1)

    def batch(t):
        b = orc.synthetic_batch(Bn, T, n_items - 1, pad_id=n_items - 1, neg=1, seed=600 + t)
        b["seq_d1"] = torch.randint(1, 120, (Bn, T), generator=g)
        b["seq_d2"] = torch.randint(120, n_items - 1, (Bn, T), generator=g)
        b["ob_label"] = (torch.rand(Bn, generator=g) < 0.6).long()
        return b

    steps = {0: 0, 1: 0}
    for epoch in range(2):
        for mode in (0, 1):
            eng.select_optimizer(mode, lr=lr if mode == 0 else lr * lr2)
            eng.dr_mode = mode
            for _ in range(3):
                steps[mode] += 1
                b = batch(10 * epoch + 5 * mode + steps[mode])
                bank_seed = seed + 0x9E3779B9 * mode
                masks = orc.philox_masks_sasrec(Bn, T, D, seed=bank_seed, step=steps[mode])
                info, _, grads = orc.dr_loss_and_grads(Po, b, "e" if mode == 0 else "r", masks, dr_e_w=w, isItC=True, threshold2=ts2)
                opts[mode].step(Po, grads)
                cu = {k: v.cuda() for k, v in b.items()}
                eng.load_batch(pl, cu["i_node"], cu["neg_samples"], cu["seq_d1"], cu["seq_d2"], cu["label"], cu["domain_id"], cu["ob_label"])
                if not eng.has_graph(pl):
                    eng.capture_train_step(pl)
                eng.replay_train_step(pl)
                eng.sync()
                got = [float(v) for v in pl.dr_losses.cpu()]
                log(f"dr traj epoch {epoch} mode {mode} step {steps[mode]}: gpu {got} oracle cls {float(info['loss_cls']):.6f} e {float(info['loss_dr_e']):.6f}")
                assert abs(got[0] - float(info["loss_cls"])) < 5e-5 and abs(got[1] - float(info["loss_dr_e"])) < 5e-5
                if mode == 1:
                    assert abs(got[2] - float(info["loss"])) < 5e-5
    eng.flush_table(); eng.sync()
    sd = eng.state_dict()
    for k, v in Po.items():
        d = (sd[k].cpu() - v).abs()
        if k.endswith("in_proj_bias"):
            Dd = v.numel() // 3
            d = torch.cat((d[:Dd], d[2 * Dd:]))
        assert float(d.max()) < 3e-4, (k, float(d.max()))


# ---------------------------------------------------------------------------- the comp modules at the batch sizes run.sh trains
def pick_open_threshold(softmaxes, B):
    """The threshold midway across the gap of the oracle's batch-softmax values with the largest margin / threshold, among the gaps that leave
    between B / 8 and 7 B / 8 gates open in every one of `softmaxes` (each the values of one of the modules that share the threshold); the
    margin is the distance from the threshold to the nearest value of any of them.  Returns (threshold, margin / threshold)."""
    sms = [s.double().reshape(-1) for s in softmaxes]
    vals = torch.cat(sms).sort().values
    best, best_t = -1.0, None
    for t in ((vals[1:] + vals[:-1]) / 2).tolist():
        if all(B <= 8 * int((s > t).sum()) <= 7 * B for s in sms):
            r = min(float((s - t).abs().min()) for s in sms) / t
            if r > best:
                best, best_t = r, t
    assert best_t is not None
    return float(best_t), best


def comp_case(variant, D, hid, T, B, seed, n_items=3000):
    """Parameters and a train batch as tests/test_gpu_eval_variants.py:oracle_case builds them: last-LayerNorm weights x 0.5 (itc) / table x 0.35
    (inc), so that the batch softmax is neither flat nor one-hot; no pad positions, so the pair-max scores are distinct."""
    itc, inc, dr = variant.startswith("itc"), variant.startswith("inc"), variant.endswith("+dr")
    P = orc.random_params(orc.sasrec_param_shapes(n_items, D, T, hid, itc_bs=B if itc else 0, dr=dr, inc_bs=B if inc else 0), seed=seed)
    if itc:
        for d in (1, 2):
            P[f"sac{d}.last_layernorm.weight"] *= 0.5
    if inc:
        P["item_emb_layer.emb_item.weight"] *= 0.35
    g = torch.Generator().manual_seed(seed + 1)
    batch = orc.synthetic_batch(B, T, n_items - 1, pad_id=n_items - 1, neg=1, seed=seed + 2)
    batch["seq_d1"] = torch.randint(1, n_items - 1, (B, T), generator=g)
    batch["seq_d2"] = torch.randint(1, n_items - 1, (B, T), generator=g)
    if dr:
        batch["ob_label"] = (torch.rand(B, generator=g) < 0.6).long()
    return P, batch


COMP_CASES = [("itc", 64, 16, 20, 32, False), ("itc", 128, 32, 20, 33, True), ("itc", 64, 16, 20, 48, True), ("itc", 128, 32, 20, 256, False),
              ("itc", 128, 32, 20, 257, False), ("itc+dr", 128, 32, 20, 256, False), ("inc", 64, 16, 20, 48, True), ("inc", 128, 32, 20, 256, False)]


@pytest.mark.parametrize("variant,D,hid,T,B,train", COMP_CASES)
def test_comp_gradients_vs_oracle_at_trained_batch_sizes(variant, D, hid, T, B, train):
    """Forward, loss and every gradient against the oracle at the batches on which InterComp's mix runs its 512-thread kernels (32 <= B <= 256, D
    64 / 128; 257: its looped form with several rows per workgroup) -- the last case is what run.sh trains -- with a threshold that opens between
    an eighth and seven eighths of the gates, chosen from the oracle's own softmax values (with the dropout masks where dropout is on) and
    at least 1 % of its value away from each of them.  The bars are those of the batch-of-8 tests above."""
    from amid_amd.engine import SasrecEngine
    itc, dr = variant.startswith("itc"), variant.endswith("+dr")
    mods = ("itc_d1", "itc_d2") if itc else ("inc_d1", "inc_d2")
    tkey = "threshold2" if itc else "threshold1"
    P, batch = comp_case(variant, D, hid, T, B, seed=60 + D)
    seed, step = 35, 2
    masks = orc.philox_masks_sasrec(B, T if itc else 2 * T, D, seed=seed, step=step) if train else None
    kw = dict(isItC=True) if itc else dict(isInC=True)
    taps = {}
    with torch.no_grad():                                        # the softmax values do not depend on the threshold
        orc.sasrec_forward(P, batch["i_node"], batch["neg_samples"], batch["seq_d1"], batch["seq_d2"], masks, taps, isDR=dr, **kw)
    ts, ratio = pick_open_threshold([taps[m]["softmax"] for m in mods], B)
    gates = [taps[m]["softmax"] > ts for m in mods]
    tag = f"comp {variant} D={D} B={B} train={train}"
    log(f"{tag}: threshold {ts:.6e} margin / threshold {ratio:.3e} open {[int(g.sum()) for g in gates]}")
    assert ratio >= 1e-2, ratio
    kw[tkey] = ts
    ekw = dict(itc_bs=B, itc_threshold=ts) if itc else dict(inc_bs=B, inc_threshold=ts)
    eng = SasrecEngine(3000, D, T, hid, lr=1e-3, seed=seed, dr=dr, **ekw)
    eng.load_state_dict(P)
    if dr:
        info, outs, grads = orc.dr_loss_and_grads(P, batch, "e", masks, dr_e_w=0.1, **kw)
        eng.dr_mode = 0
        pl = eng.plan(B, T, 2, need_grad=True)
        eng.set_step(step, seed)
        cu = {k: v.cuda() for k, v in batch.items()}
        eng.load_batch(pl, cu["i_node"], cu["neg_samples"], cu["seq_d1"], cu["seq_d2"], cu["label"], cu["domain_id"], cu["ob_label"])
        eng.enqueue_prepare(pl, sparse=True)
        eng.enqueue_forward(pl, train=train, with_loss=True)
        eng.enqueue_backward(pl, train=train)
        eng.sync()
        eng.check_index_error(pl)
        assert torch.equal(pl.itc_gate.cpu(), gates[0].float())
        for name, got, want in zip(("p1", "p2", "ips1", "ips2", "g1", "g2"), (pl.p1, pl.p2, pl.ips1, pl.ips2, pl.g1, pl.g2), outs):
            e = relmax(got, want)
            log(f"{tag} {name} relmax {e:.3e}")
            assert e < 3e-5, (name, e)
        lc, le, _ = (float(v) for v in pl.dr_losses.cpu())
        log(f"{tag} loss_cls {lc:.7f} (oracle {float(info['loss_cls']):.7f}) loss_dr_e {le:.7f} (oracle {float(info['loss_dr_e']):.7f})")
        assert abs(lc + 0.1 * le - float(info["loss"])) < 1e-5
        dr_grads_check(tag, eng, pl, grads, 5e-4)
        return
    loss, (p1, p2), grads = orc.loss_and_grads("sasrec", P, batch, masks, **kw)
    pl = run_forward(eng, batch, train=train, with_loss=True, step=step, seed=seed)
    if itc:
        assert torch.equal(pl.itc_gate.cpu(), gates[0].float())
    else:
        for d in (0, 1):
            assert torch.equal(pl.inc_gate[d].cpu(), gates[d].float())
    e1, e2 = relmax(pl.p1, p1), relmax(pl.p2, p2)
    log(f"{tag} p1 relmax {e1:.3e} p2 relmax {e2:.3e}")
    assert e1 < 3e-5 and e2 < 3e-5
    eng.enqueue_backward(pl, train=train)
    eng.sync()
    assert abs(float(pl.loss.item()) - float(loss)) < 1e-5
    grads_check(tag, eng, pl, grads, 5e-4 if train else 2e-4, 5e-3 if train else 2e-4)


def test_itc_train_step_vs_oracle_dense_adam():
    """Three isItC train steps (dropout on) at a batch of 48 -- the mix's 512-thread forward and backward -- against the oracle's dense Adam:
    losses and the parameters after the steps, InterComp's included; eager and graph replay bit-identical.  The pair-max scores move with every
    step's dropout masks, so the threshold is one that keeps 1 % of its value from the oracle's softmax values of all three steps."""
    D, T, B, hid = 64, 20, 48, 16
    P, batch = comp_case("itc", D, hid, T, B, seed=60 + D)
    seed, lr = 5, 1e-3

    # A step's softmax values depend on the threshold only through the gates of the steps before it.  So the threshold is narrowed step by
    # step: (lo, hi) holds no softmax value of the steps so far -- any threshold in it gives them the same gates --, the next step's values
    # split it, and the parts that keep 1 % of their midpoint on either side and open an eighth to seven eighths of that step's gates are
    # tried widest first; a part that leaves a later step no such part is dropped for the next one.
    def narrow(Pref, opt, t, lo, hi):
        if t == 4:
            return Pref, (lo + hi) / 2, [], []
        masks = orc.philox_masks_sasrec(B, T, D, seed=seed, step=t)
        taps = {}
        with torch.no_grad():
            orc.sasrec_forward(Pref, batch["i_node"], batch["neg_samples"], batch["seq_d1"], batch["seq_d2"], masks, taps, isItC=True)
        sm = torch.cat((taps["itc_d1"]["softmax"], taps["itc_d2"]["softmax"])).double()      # (both directions' values, equal up to rounding)
        edges = [lo] + sorted(v for v in sm.tolist() if lo < v < hi) + [hi]
        parts = [(a, b) for a, b in zip(edges[:-1], edges[1:])
                 if (b - a) / (b + a) >= 1e-2 and 2 * B <= 8 * int((sm > (a + b) / 2).sum()) <= 2 * 7 * B]
        for a, b in sorted(parts, key=lambda p: (p[1] - p[0]) / (p[1] + p[0]), reverse=True):
            Pn, on = {k: v.clone() for k, v in Pref.items()}, copy.deepcopy(opt)
            loss = orc.train_step("sasrec", Pn, on, batch, masks, isItC=True, threshold2=(a + b) / 2)
            r = narrow(Pn, on, t + 1, a, b)
            if r is not None:
                return r[0], r[1], [loss] + r[2], [sm] + r[3]
        return None

    P0 = {k: v.clone() for k, v in P.items()}
    found = narrow(P0, orc.DenseAdam(P0, lr=lr), 1, 0.0, 1.0)
    assert found is not None
    Pref, ts, ref_losses, sms = found
    ratio = min(float((s - ts).abs().min()) for s in sms) / ts
    n_open = [int((s > ts).sum()) // 2 for s in sms]
    log(f"itc dense-adam B={B}: threshold {ts:.6e} margin / threshold {ratio:.3e} open {n_open}")
    assert ratio >= 1e-2 and all(B <= 8 * n <= 7 * B for n in n_open)

    def run(use_graph):
        eng = make_itc_engine(P, T, B, ts, lr=lr, seed=seed)
        pl = eng.plan(B, T, 2, need_grad=True)
        cu = {k: v.cuda() for k, v in batch.items()}
        eng.load_batch(pl, cu["i_node"], cu["neg_samples"], cu["seq_d1"], cu["seq_d2"], cu["label"], cu["domain_id"])
        if use_graph:
            eng.capture_train_step(pl)
        losses = []
        for _ in range(3):
            eng.replay_train_step(pl) if use_graph else eng.enqueue_train_step(pl)
            eng.sync()
            losses.append(float(pl.loss.item()))
        eng.flush_table(); eng.sync()
        return losses, {k: v.cpu().clone() for k, v in eng.state_dict().items()}
    l0, s0 = run(False)
    l1, s1 = run(True)
    assert l0 == l1 and all(torch.equal(s0[k], s1[k]) for k in s0)
    for a, b in zip(l0, ref_losses):
        assert abs(a - float(b)) < 2e-5
    for k, v in Pref.items():
        d = (s0[k] - v).abs()
        if k.endswith("in_proj_bias"):
            Dd = v.numel() // 3
            d = torch.cat((d[:Dd], d[2 * Dd:]))      # chaotic key-bias slice, see test_oracle_golden
        log(f"itc dense-adam B={B} {k:50s} max |diff| {float(d.max()):.3e}")
        assert float(d.max()) < 2e-4, (k, float(d.max()))


# ---------------------------------------------------------------------------- edge shapes (ragged / empty / maximum inputs)
@pytest.mark.parametrize("Bn,T,D,neg", [(1, 50, 128, 1), (3, 7, 64, 4), (5, 64, 128, 1), (4, 70, 64, 2), (2, 1, 64, 1), (512, 50, 128, 1),
                                         (16, 20, 128, 999), (3, 150, 128, 1)])
def test_edge_shapes_forward_backward_vs_oracle(Bn, T, D, neg):
    """One row, odd small shapes, T at the matrix-core attention limit (64) and beyond it (70: general kernel), a single time
    step, the cfg 3 batch (512 x 50), the evaluation fan-out of run.sh (999 negatives) and the reference's amazon sequence length
    (train_sr_dr.py:550: 150; attention in two head groups per sequence); some rows entirely padding (an empty
    history in one or both domains) and some with no padding at all."""
    hid, n_items = 16, 700
    P = orc.random_params(orc.sasrec_param_shapes(n_items, D, T, hid), seed=Bn + T)
    batch = orc.synthetic_batch(Bn, T, n_items - 1, pad_id=n_items - 1, neg=neg, seed=Bn * 7 + T, mean_len=min(5.0, T))
    batch["seq_d1"][0] = n_items - 1                          # empty history in domain 1
    if Bn > 1:
        batch["seq_d2"][1] = n_items - 1                      # empty history in domain 2
        batch["seq_d1"][1] = torch.arange(1, T + 1)           # full-length history
    if Bn > 2:
        batch["seq_d1"][2] = n_items - 1
        batch["seq_d2"][2] = n_items - 1                      # nothing at all
    eng = make_engine(P, T, seed=3)
    pl = run_forward(eng, batch, train=False, with_loss=True)
    p1, p2 = orc.sasrec_forward(P, batch["i_node"], batch["neg_samples"], batch["seq_d1"], batch["seq_d2"])
    assert relmax(pl.p1, p1) < 3e-5 and relmax(pl.p2, p2) < 3e-5
    if Bn <= 16 and neg <= 4:
        loss, _, grads = orc.loss_and_grads("sasrec", P, batch, None)
        eng.enqueue_backward(pl, train=False)
        eng.sync()
        assert abs(float(pl.loss.item()) - float(loss)) < 1e-5
        taps = {}
        orc.sasrec_forward({k: v.double() for k, v in P.items()}, batch["i_node"], batch["neg_samples"], batch["seq_d1"], batch["seq_d2"], None, taps)
        margin = min(taps[s][f"relu_margin{l}"] for s in ("sac1", "sac2") for l in (0, 1))
        tol = 3e-4 if margin > 2e-5 else 5e-2
        grads_check(f"edge B={Bn} T={T} D={D}", eng, pl, grads, tol, 3e-4 if margin > 2e-5 else 1e-2)


@pytest.mark.parametrize("Bn,D,train", [(256, 128, True), (256, 64, False), (128, 128, True), (160, 64, False)])
def test_headline_shape_forward_backward_vs_oracle(Bn, D, train):
    """BASELINE.json configs[1] itself (B 256, T 50) and smaller batches, forward + backward through the PLAIN kernels (both domains of
    every sample, as model.forward encodes them) against the oracle, dropout on.  At this size some relu pre-activation always sits within rounding of the kink, so the oracle is given
    the kernels' own relu decisions (relu_keep; every decision that differs from the oracle's own must be rounding-sized) and the
    gradients are held to max-abs 2e-4."""
    T, hid, n_items = 50, 32, 3000
    P = orc.random_params(orc.sasrec_param_shapes(n_items, D, T, hid), seed=90 + D)
    batch = orc.synthetic_batch(Bn, T, n_items - 1, pad_id=n_items - 1, neg=1, seed=77)
    seed, step = 21, 4
    masks = orc.philox_masks_sasrec(Bn, T, D, seed=seed, step=step) if train else None
    eng = make_engine(P, T, seed=seed)
    pl = run_forward(eng, batch, train=train, with_loss=True, step=step, seed=seed)
    assert pl.rt_suffix == "" and pl.rpt == -(-2 * Bn * T // 256)
    eng.enqueue_backward(pl, train=train)
    eng.sync()
    M = Bn * T
    keep = {f"sac{g + 1}.relu{l}": (pl.h[l][g * M:(g + 1) * M].reshape(Bn, T, D).cpu() > 0).float() for g in (0, 1) for l in (0, 1)}
    taps = {}
    loss, (p1, p2), grads = orc.loss_and_grads("sasrec", P, batch, masks, relu_keep=keep, taps=taps)
    assert max(taps[s_].get(f"relu_flip{l}", 0.0) for s_ in ("sac1", "sac2") for l in (0, 1)) < 2e-5
    assert relmax(pl.p1, p1) < 1e-4 and relmax(pl.p2, p2) < 1e-4
    assert abs(float(pl.loss.item()) - float(loss)) < 1e-5
    for name in eng.dense.slots:
        got, want = eng.dense.view(name, eng.dense.grad), grads[name]
        if name.endswith("in_proj_bias"):
            n3 = got.numel() // 3
            got, want = got.cpu().clone(), want.clone()
            got[n3:2 * n3] = 0; want[n3:2 * n3] = 0
        assert relmax(got, want) < 2e-4 and rel_l2(got, want) < 5e-5, (name, relmax(got, want), rel_l2(got, want))
    tg = dense_table_grad(eng, pl)
    assert relmax(tg, grads["item_emb_layer.emb_item.weight"]) < 2e-4 and rel_l2(tg, grads["item_emb_layer.emb_item.weight"]) < 5e-5


# ---------------------------------------------------------------------------- bf16 matrix products (BASELINE.json configs[2])
def test_bf16_compute_within_tolerance_of_fp32_oracle():
    """compute="bf16": bf16 MFMA operands, fp32 accumulation / storage / everything else, at the cfg-3 batch (512 x 50 x 128):
    logits within 2e-2 relative of the fp32 oracle, gradients close in the L2 sense, training moves the loss."""
    from amid_amd.engine import SasrecEngine
    D, T, Bn, hid, n_items = 128, 50, 512, 32, 3000
    P = orc.random_params(orc.sasrec_param_shapes(n_items, D, T, hid), seed=91)
    batch = orc.synthetic_batch(Bn, T, n_items - 1, pad_id=n_items - 1, neg=1, seed=17)
    eng = SasrecEngine(n_items, D, T, hid, lr=1e-3, seed=4, compute="bf16")
    eng.load_state_dict(P)
    pl = run_forward(eng, batch, train=False, with_loss=True)
    p1, p2 = orc.sasrec_forward(P, batch["i_node"], batch["neg_samples"], batch["seq_d1"], batch["seq_d2"])
    e1, e2 = relmax(pl.p1, p1), relmax(pl.p2, p2)
    log(f"bf16 cfg3 logits relmax {e1:.3e} {e2:.3e}")
    assert e1 < 2e-2 and e2 < 2e-2
    assert e1 > 1e-5                                   # the mode is really on (fp32 products land at ~1e-6)
    sub = {k: v[:32] for k, v in batch.items()}        # gradients on a slice the oracle differentiates quickly
    eng2 = SasrecEngine(n_items, D, T, hid, lr=1e-3, seed=4, compute="bf16")
    eng2.load_state_dict(P)
    pl2 = run_forward(eng2, sub, train=False, with_loss=True)
    eng2.enqueue_backward(pl2, train=False)
    eng2.sync()
    loss, _, grads = orc.loss_and_grads("sasrec", P, sub, None)
    assert abs(float(pl2.loss.item()) - float(loss)) < 2e-3
    worst = 0.0
    for name in eng2.dense.slots:
        if name.endswith("in_proj_bias"):
            continue
        e = rel_l2(eng2.dense.view(name, eng2.dense.grad), grads[name])
        worst = max(worst, e)
        assert e < 6e-2, (name, e)
    log(f"bf16 grads worst rel L2 {worst:.3e}")
    assert rel_l2(dense_table_grad(eng2, pl2), grads["item_emb_layer.emb_item.weight"]) < 6e-2
    # a few train steps (dropout on, graph replay): the loss goes down and stays close to the fp32 engine's
    ref = make_engine(P, T, lr=1e-3, seed=4)
    losses = {}
    for key, e in (("bf16", eng), ("f32", ref)):
        q = e.plan(Bn, T, 2, need_grad=True)
        cu = {k: v.cuda() for k, v in batch.items()}
        e.load_batch(q, cu["i_node"], cu["neg_samples"], cu["seq_d1"], cu["seq_d2"], cu["label"], cu["domain_id"])
        e.capture_train_step(q)
        ls = []
        for _ in range(5):
            e.replay_train_step(q)
            e.sync()
            ls.append(float(q.loss.item()))
        losses[key] = ls
    log(f"bf16 train losses {losses}")
    assert losses["bf16"][-1] < losses["bf16"][0]
    assert all(abs(a - b) < 5e-3 for a, b in zip(losses["bf16"], losses["f32"]))
