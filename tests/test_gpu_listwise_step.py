"""Train steps on K sampled negatives under the listwise objectives (loss = "softmax" | "bpr": DESIGN.md section 17), engine level.

1. One eval-mode enqueue_forward + enqueue_backward of SASRec plain, SASRec isItC (batch = bs), BERT4Rec plain and GRU4Rec plain against
   the oracle in float64 -- orc.sasrec_forward, orc.bert4rec_forward, tests/gru_ref.py -- with the objective written on logit(p)
   (tests/listwise_ref.py loss_on_p) and torch.autograd: the loss, the table's unique-row gradients and every dense gradient, at the bars
   the BCE step's comparisons use in tests/test_gpu_sasrec.py (loss 1e-5 max(1, |loss|), gradients 2e-4 max / 2e-4 l2 with the encoders'
   ReLU margin over 2e-5), test_gpu_bert4rec.py (the same) and test_gpu_gru4rec.py (loss 1e-5, gradients 5e-4 / 5e-4).
   predictModule's bias fc.2.bias takes no gradient from either objective (they do not change when every logit moves alike): its gradient
   is rounding noise on both sides and is held against fc.0.bias's largest entry, the way the key bias is in those files.
2. loss = "bce" at K 4 and 64 against orc.loss_and_grads, the same bars: NI > 2 in training.
3. Train steps with dropout on through a 2-step graph over an input pool against eager steps: parameters torch.equal.
4. The default model and loss = "bce" on one-negative batches: parameters torch.equal after three steps.
5. The refusals.  6. The command line in fresh processes."""
import re

import pytest
import torch

from oracle import amid_oracle as orc
from tests import gru_ref
from tests import listwise_ref as LW
from tests.test_gpu_sasrec import dense_table_grad, log, rel_l2, relmax

pytestmark = pytest.mark.gpu
F64 = torch.float64
HID, N_ITEMS = 32, 400


@pytest.fixture(autouse=True)
def stop_at_a_gpu_fault():
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the GPU reported an error, nothing more is launched: {e}", returncode=3)


# ---------------------------------------------------------------------------- models: parameters, batch, float64 forward, engine
def sasrec_setup(B, T, D, K, itc):
    """isItC: the parameter seed is stepped (at most 8 times) until the gate is neither empty nor full with its softmax margin over 1e-3 in
    float64 (test_gpu_sasrec.test_itc_vs_oracle_and_train_steps' conditions).  The gradient bars follow test_backward_grads_vs_oracle's rule:
    2e-4 when every encoder ReLU pre-activation is farther than 2e-5 from 0, else 5e-2 max / 1e-2 l2 (at 32 rows a few of the 300 000
    pre-activations always are nearer; a flipped unit is a discrete error of one row's size)."""
    kw = dict(isItC=True, threshold2=0.03) if itc else {}
    batch = orc.synthetic_batch(B, T, N_ITEMS - 1, pad_id=N_ITEMS - 1, neg=K, seed=4 + K)
    if itc:
        g = torch.Generator().manual_seed(7)
        batch["seq_d1"] = torch.randint(1, N_ITEMS - 1, (B, T), generator=g)      # no shared pad positions: distinct pair-max scores
        batch["seq_d2"] = torch.randint(1, N_ITEMS - 1, (B, T), generator=g)
    for step in range(9):
        P = orc.random_params(orc.sasrec_param_shapes(N_ITEMS, D, T, HID, **(dict(itc_bs=B) if itc else {})), seed=60 + D + T + 1000 * step)
        if itc:
            for d in (1, 2):
                P[f"sac{d}.last_layernorm.weight"] *= 0.3          # keeps the batch softmax of the pair-max scores away from one-hot
        taps = {}
        orc.sasrec_forward({k: v.double() for k, v in P.items()}, batch["i_node"], batch["neg_samples"], batch["seq_d1"], batch["seq_d2"], None, taps, **kw)
        margin = min(taps[s][f"relu_margin{l}"] for s in ("sac1", "sac2") for l in (0, 1))
        if not itc or (0 < int(taps["itc_d1"]["gate"].sum()) < B and taps["itc_d1"]["margin"] > 1e-3):
            break
    else:
        raise AssertionError("no parameter seed within 8 steps meets the gate conditions")
    print(f"sasrec setup B {B} T {T} D {D} itc {itc}: seed step {step}, encoder relu margin {margin:.3e}")
    fwd = lambda L_: orc.sasrec_forward(L_, batch["i_node"], batch["neg_samples"], batch["seq_d1"], batch["seq_d2"], None, **kw)      # noqa: E731

    def engine(loss):
        from amid_amd.engine import SasrecEngine
        e = SasrecEngine(N_ITEMS, D, T, HID, lr=1e-3, seed=3, loss=loss, **(dict(itc_bs=B, itc_threshold=0.03) if itc else {}))
        e.load_state_dict(P)
        return e
    return P, batch, fwd, engine, 1e-5, (2e-4, 2e-4) if margin > 2e-5 else (5e-2, 1e-2)


def bert_setup(B, T, D, K, itc):
    from tests.test_gpu_bert4rec import batch_with_masked_keys
    P = orc.random_params(orc.bert4rec_param_shapes(N_ITEMS, HID), seed=70 + T)
    batch = batch_with_masked_keys(B, T, N_ITEMS, seed=5 + K, neg=K)
    fwd = lambda L_: orc.bert4rec_forward(L_, batch["i_node"], batch["neg_samples"], batch["seq_d1"], batch["seq_d2"], None)      # noqa: E731

    def engine(loss):
        from amid_amd.engine_bert import Bert4recEngine
        e = Bert4recEngine(N_ITEMS, 128, T, HID, lr=1e-3, seed=3, loss=loss)
        e.load_state_dict(P)
        return e
    return P, batch, fwd, engine, 1e-5, (2e-4, 2e-4)


def gru_setup(B, T, D, K, itc):
    P = orc.random_params(gru_ref.gru4rec_param_shapes(N_ITEMS, 128, HID), seed=80 + T)
    batch = orc.synthetic_batch(B, T, N_ITEMS - 1, pad_id=N_ITEMS - 1, neg=K, seed=6 + K)
    fwd = lambda L_: gru_ref.gru4rec_forward(L_, batch["i_node"], batch["neg_samples"], batch["seq_d1"], batch["seq_d2"])      # noqa: E731

    def engine(loss):
        from amid_amd.engine_gru import Gru4recEngine
        e = Gru4recEngine(N_ITEMS, 128, T, HID, lr=1e-3, seed=3, loss=loss)
        e.load_state_dict(P)
        return e
    return P, batch, fwd, engine, 1e-5, (5e-4, 5e-4)


SETUPS = {"sasrec": sasrec_setup, "sasrec_itc": sasrec_setup, "bert4rec": bert_setup, "gru4rec": gru_setup}


def oracle(P, fwd, batch, loss):
    """(loss, grads) in float64 by autograd: the model's forward, then the objective on logit(p) -- or the masked BCE."""
    leaves = {k: v.detach().double().clone().requires_grad_(True) for k, v in P.items()}
    p1, p2 = fwd(leaves)
    if loss == "bce":
        val = orc.masked_bce_loss(p1, p2, batch["label"].double(), batch["domain_id"])
    else:
        val = LW.loss_on_p(p1, p2, batch["domain_id"], LW.KINDS[loss])
    names = list(leaves)
    gs = torch.autograd.grad(val, [leaves[n] for n in names], allow_unused=True)
    return float(val.detach()), {n: (g if g is not None else torch.zeros_like(leaves[n])) for n, g in zip(names, gs)}


def run_engine(eng, batch):
    Bn, T = batch["seq_d1"].shape
    pl = eng.plan(Bn, T, 1 + batch["neg_samples"].shape[1], need_grad=True)
    cu = {k: v.cuda() for k, v in batch.items()}
    eng.load_batch(pl, cu["i_node"], cu["neg_samples"], cu["seq_d1"], cu["seq_d2"], cu["label"], cu["domain_id"])
    eng.enqueue_prepare(pl, sparse=True)
    eng.enqueue_forward(pl, train=False, with_loss=True)
    eng.enqueue_backward(pl, train=False)
    eng.sync()
    eng.check_index_error(pl)
    return pl


def compare(tag, eng, pl, loss, grads, loss_tol, tol, listwise):
    got = float(pl.loss.item())
    print(f"{tag}: loss {got:.7f} oracle {loss:.7f}")
    log(f"{tag}: loss {got:.7f} oracle {loss:.7f}")
    bad = []
    if not abs(got - loss) < loss_tol * max(1.0, abs(loss)):
        bad.append(("loss", got, loss))
    for name in list(eng.dense.slots) + ["item_emb_layer.emb_item.weight"]:
        g = dense_table_grad(eng, pl) if name.startswith("item_emb") else eng.dense.view(name, eng.dense.grad).cpu().clone()
        w = grads[name].clone()
        if name.endswith("in_proj_bias"):            # the key-bias third is analytically zero (test_gpu_sasrec.grads_check)
            D = g.numel() // 3
            g[D:2 * D] = 0; w[D:2 * D] = 0
        if name.endswith("linear_layers.1.bias") or (listwise and name == "predictModule.fc.2.bias"):
            # analytically zero (BERT4Rec's key bias; the listwise objectives' common shift of the logits): rounding noise on both sides
            ref = grads[name.replace("linear_layers.1", "linear_layers.0") if "linear_layers" in name else "predictModule.fc.0.bias"].abs().max()
            if not float(g.abs().max()) < 1e-4 * float(ref) + 1e-9:
                bad.append((name, float(g.abs().max()), float(ref)))
            continue
        e, e2 = relmax(g, w), rel_l2(g, w)
        print(f"{tag} grad {name:50s} relmax {e:.3e} l2 {e2:.3e}")
        log(f"{tag} grad {name:50s} relmax {e:.3e} l2 {e2:.3e}")
        if not (e < tol[0] and e2 < tol[1]):
            bad.append((name, e, e2))
    assert not bad, (tag, bad)


CASES = [(m, T, K, 128) for m in SETUPS for T in (8, 20) for K in (4, 64)] + [("sasrec", 20, 4, 64), ("sasrec", 8, 64, 64)]


@pytest.mark.parametrize("loss", ["softmax", "bpr"])
@pytest.mark.parametrize("model,T,K,D", CASES)
def test_listwise_step_against_the_float64_oracle(model, T, K, D, loss):
    B = 32 if model == "sasrec_itc" else 8
    P, batch, fwd, engine, loss_tol, tol = SETUPS[model](B, T, D, K, model == "sasrec_itc")
    want, grads = oracle(P, fwd, batch, loss)
    eng = engine(loss)
    pl = run_engine(eng, batch)
    # the other domain's logits carry no gradient, exactly
    oth = 1 - (batch["domain_id"] != 0).long()
    dz = torch.stack((pl.dp1.cpu(), pl.dp2.cpu()))
    assert torch.equal(dz[oth, torch.arange(B)], torch.zeros(B, 1 + K))
    compare(f"listwise {model} {loss} T {T} K {K} D {D}", eng, pl, want, grads, loss_tol, tol, True)


@pytest.mark.parametrize("model,T,K,D", [("sasrec", 20, 4, 128), ("sasrec", 8, 64, 128), ("sasrec", 20, 64, 64), ("bert4rec", 20, 64, 128),
                                         ("gru4rec", 8, 4, 128), ("gru4rec", 20, 64, 128), ("sasrec_itc", 20, 64, 128)])
def test_bce_step_with_several_negatives(model, T, K, D):
    """loss = "bce" beyond one negative (the general forms of the existing heads): NI 5 and 65 against orc.loss_and_grads' arithmetic."""
    B = 32 if model == "sasrec_itc" else 8
    P, batch, fwd, engine, loss_tol, tol = SETUPS[model](B, T, D, K, model == "sasrec_itc")
    want, grads = oracle(P, fwd, batch, "bce")
    if model == "sasrec":                       # (the float64 oracle above is orc.loss_and_grads' computation: held to it where that exists in fp32)
        l32, _, _ = orc.loss_and_grads("sasrec", P, batch, None)
        assert abs(float(l32) - want) < 1e-5
    eng = engine("bce")
    compare(f"bce {model} T {T} K {K} D {D}", eng, run_engine(eng, batch), want, grads, loss_tol, tol, False)


# ---------------------------------------------------------------------------- whole train steps through the models
def epoch(n, B, T, K, seed):
    g = torch.Generator().manual_seed(seed)
    pad = N_ITEMS - 1

    def seq():
        ids = torch.randint(1, 300, (n, B, T), generator=g)
        n_pad = torch.randint(0, T, (n, B, 1), generator=g)
        return torch.where(torch.arange(T) < n_pad, torch.full_like(ids, pad), ids)
    label = torch.zeros(B, 1 + K)
    label[:, 0] = 1.0
    ep = dict(i_node=torch.randint(1, 300, (n, B), generator=g), neg_samples=torch.randint(1, 300, (n, B, K), generator=g), seq_d1=seq(),
              seq_d2=seq(), domain_id=torch.randint(0, 2, (n, B), generator=g), label=label)
    return {k: v.cuda() for k, v in ep.items()}


def make_model(kind, B, T, **kw):
    from amid_amd.model_gru import GRU4Rec
    from amid_amd.model_seq import BERT4Rec, SASRec
    cls = {"sasrec": SASRec, "sasrec_itc": SASRec, "bert4rec": BERT4Rec, "gru4rec": GRU4Rec}[kind]
    return cls(10, 128, N_ITEMS, 128, T, HID, B, False, kind == "sasrec_itc", 0.5, 0.03, lr=1e-3, seed=5, **kw)


def flushed(m):
    m.engine.flush_table()
    m.engine.sync()
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}


@pytest.mark.parametrize("kind,loss,K", [("sasrec", "softmax", 4), ("sasrec", "bpr", 64), ("sasrec_itc", "softmax", 4), ("bert4rec", "softmax", 64),
                                         ("gru4rec", "bpr", 4), ("sasrec", "bce", 4), ("sasrec", "bce", 64), ("bert4rec", "bce", 64)])
def test_pooled_two_step_graph_equals_eager_steps(kind, loss, K):
    """Four train steps, dropout on: two replays of a 2-step graph over the input pool against four eager pool steps.  loss = "bce" rides
    along at K 4 (the folded step at NI 5) and K 64 (NI 65: past the folded step's one item chunk, the general heads)."""
    B, T, n = (32 if kind == "sasrec_itc" else 8), 20, 4
    ep = epoch(n, B, T, K, seed=21)
    out = []
    for graph in (True, False):
        m = make_model(kind, B, T, loss=loss)
        m.train()
        m.begin_epoch_pool(ep)
        losses = []
        for _ in range(n // 2 if graph else n):
            v = m.pool_step(n_steps=2) if graph else m.pool_step(use_graph=False)
            m.engine.sync()
            losses.append(float(v.item()))
        m.end_epoch_pool()
        out.append((losses, flushed(m)))
    (lg, sg), (le, se) = out
    assert all(map(lambda x: x == x and abs(x) < 1e3, lg + le)), (lg, le)
    assert lg == le[1::2], (lg, le)
    assert all(torch.equal(sg[k], se[k]) for k in sg), [k for k in sg if not torch.equal(sg[k], se[k])]


def test_default_model_is_the_bce_model():
    """SASRec(...) without the new keyword and SASRec(..., loss="bce") on one-negative batches: the same parameters after three steps."""
    B, T = 8, 20
    ep = epoch(3, B, T, 1, seed=22)
    sd = []
    for kw in ({}, {"loss": "bce"}):
        m = make_model("sasrec", B, T, **kw)
        m.train()
        for i in range(3):
            m.train_step(ep["i_node"][i], ep["neg_samples"][i], ep["seq_d1"][i], ep["seq_d2"][i], ep["label"], ep["domain_id"][i])
        sd.append(flushed(m))
    assert all(torch.equal(sd[0][k], sd[1][k]) for k in sd[0])


def test_listwise_steps_lower_the_loss():
    """Thirty softmax steps on one batch: the loss falls from about log(1 + K)."""
    B, T, K = 8, 20, 16
    ep = epoch(1, B, T, K, seed=23)
    m = make_model("sasrec", B, T, loss="softmax")
    m.train()
    ls = []
    for _ in range(30):
        v = m.train_step(ep["i_node"][0], ep["neg_samples"][0], ep["seq_d1"][0], ep["seq_d2"][0], ep["label"], ep["domain_id"][0])
        m.engine.sync()
        ls.append(float(v.item()))
    print("softmax losses", ls[0], ls[-1])
    assert ls[-1] < 0.8 * ls[0] and all(x == x for x in ls)


# ---------------------------------------------------------------------------- refusals
def test_refusals():
    from amid_amd.engine import SasrecEngine
    from amid_amd.engine_bert import Bert4recEngine
    from amid_amd.engine_gru import Gru4recEngine
    from amid_amd.model_gru import GRU4RecAMID
    from amid_amd.model_seq import BERT4Rec, SASRec
    with pytest.raises(ValueError, match="loss must be"):
        SasrecEngine(N_ITEMS, 128, 20, HID, loss="hinge")
    with pytest.raises(ValueError, match="isDR"):
        SasrecEngine(N_ITEMS, 128, 20, HID, dr=True, loss="softmax")
    with pytest.raises(ValueError, match="bf16"):
        SasrecEngine(N_ITEMS, 128, 20, HID, compute="bf16", loss="bpr")
    with pytest.raises(ValueError, match="isInC"):
        SasrecEngine(N_ITEMS, 128, 20, HID, inc_bs=8, loss="softmax")
    with pytest.raises(ValueError, match="comp module"):
        Bert4recEngine(N_ITEMS, 128, 20, HID, comp="itc", comp_bs=8, loss="softmax")
    with pytest.raises(ValueError, match="isItC"):
        Gru4recEngine(N_ITEMS, 128, 20, HID, itc_bs=8, loss="softmax")
    with pytest.raises(ValueError, match="isDR"):
        SASRec(10, 128, N_ITEMS, 128, 20, HID, 8, False, False, 0.5, 0.5, isDR=True, loss="softmax")
    with pytest.raises(ValueError):
        BERT4Rec(10, 128, N_ITEMS, 128, 20, HID, 8, True, False, 0.5, 0.5, loss="bpr")
    with pytest.raises(ValueError):
        GRU4RecAMID(10, 128, N_ITEMS, 128, 20, HID, 8, False, True, 0.5, 0.5, loss="bpr")

    class World2:                                # an exchange over two ranks: refused before anything is exchanged
        world, active, grad_scale = 2, True, 0.5
    eng = SasrecEngine(N_ITEMS, 128, 20, HID, loss="softmax")
    pl = eng.plan(8, 20, 5, need_grad=True)
    with pytest.raises(ValueError, match="data-parallel"):
        eng.train_step_dp(pl, World2())


# ---------------------------------------------------------------------------- the command line, in fresh processes
def test_cli_trains_with_softmax_and_refuses_a_resume_under_another_loss(tmp_path):
    import subprocess
    import sys
    from tests.test_gpu_checkpoint import ROOT, _cli, _data, _log
    base = _data(tmp_path, False) + ["--seeds", "1", "--epoch", "1", "--max_steps", "3", "--train_negs", "4"]
    save, logs = tmp_path / "S", tmp_path / "logs"
    _cli("amid_amd.train_sr", base + ["--loss", "softmax", "--save_dir", str(save), "-md", str(logs)])
    lines = _log(logs / "log0.txt")
    assert any("'train_negs': 4" in ln and "'loss': 'softmax'" in ln for ln in lines)
    vals = [float(x) for ln in lines if ln.startswith("train total loss:") for x in re.findall(r"total loss:([-+0-9.eE]+|nan|inf)", ln)]
    assert vals and all(v == v and abs(v) < 1e3 for v in vals), vals
    r = subprocess.run([sys.executable, "-m", "amid_amd.train_sr"] + base + ["--loss", "bpr", "--resume", str(save / "seed0" / "last.pt"), "-md", str(logs)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--loss" in r.stderr and "'softmax'" in r.stderr, r.stderr[-2000:]
