"""Train steps with hard-negative mining (hard_negs = H > 0, hard_skip = S: DESIGN.md section 18), engine and model level, in the manner of
tests/test_gpu_listwise_step.py and at its smallest shapes: hard_negs 2 of 6 drawn negatives, hard_skip 1, both objectives, SASRec plain,
SASRec isItC (batch = bs), BERT4Rec plain and GRU4Rec plain.  The float64 oracle is the model's forward, the objective on logit(p) of the
columns [0] + sel (tests/mined_ref.py loss_on_p) and torch.autograd, with the selection READ BACK from pl.sel: the selection is a constant of
the step, and which of two logits closer than a float32 rounding ranks first is not the oracle's to decide (tests/test_gpu_mined.py holds the
selection itself to the rule).

1. One eval-mode forward + backward: the loss, every dense gradient and the table's gradient -- the rows of the candidates that were not
   kept included: exactly the gradient their other uses in the batch give them, zero if none -- at test_gpu_listwise_step.py's bars.
2. One whole train step (dropout on, the kernels' Philox masks in the oracle; Adam): the loss, every dense parameter and the whole table
   against orc.DenseAdam on the dense gradient.  A candidate that was not kept stays in the step's index list with a zero gradient: under
   dense Adam from zero moments its row does not move and its moments stay zero, which is checked exactly on the rows that the batch
   uses as non-kept candidates only.  Bars: loss 5e-5 max(1, |loss|), parameters 1e-4, table 1e-5 relative (tests/test_gpu_optim.py
   check_params; one Adam step moves a parameter by about lr = 1e-3).  predictModule.fc.2.bias takes no gradient from either objective;
   Adam normalises the rounding noise left in its place, so it is only held to |move| <= lr (as the key biases are left out there).
3. A pooled 2-step graph replay is bit-equal to eager pool steps.  4. hard_negs = 0 gives the bits of an engine built without the keyword.
5. The refusals, the first-step one included.  6. train_sr.py with the flags in a fresh process: the epoch's log line."""
import math
import re

import pytest
import torch

from oracle import amid_oracle as orc
from tests import gru_ref
from tests import listwise_ref as LW
from tests import mined_ref as MR
from tests.test_gpu_listwise_step import HID, N_ITEMS, SETUPS, compare, epoch, flushed, make_model, run_engine, stop_at_a_gpu_fault  # noqa: F401
from tests.test_gpu_sasrec import log

pytestmark = pytest.mark.gpu
F64 = torch.float64
K, H, S, T = 6, 2, 1, 8
TABLE = "item_emb_layer.emb_item.weight"
MODELS = ["sasrec", "sasrec_itc", "bert4rec", "gru4rec"]


def make_engine(model, P, B, loss, seed=3, **kw):
    from amid_amd.engine import SasrecEngine
    from amid_amd.engine_bert import Bert4recEngine
    from amid_amd.engine_gru import Gru4recEngine
    cls = {"sasrec": SasrecEngine, "sasrec_itc": SasrecEngine, "bert4rec": Bert4recEngine, "gru4rec": Gru4recEngine}[model]
    e = cls(N_ITEMS, 128, T, HID, lr=1e-3, seed=seed, loss=loss, **(dict(itc_bs=B, itc_threshold=0.03) if model == "sasrec_itc" else {}), **kw)
    e.load_state_dict(P)
    return e


def mined_oracle(P, fwd, batch, loss, sel):
    """(loss, grads) in float64 by autograd on the columns [0] + sel."""
    leaves = {k: v.detach().double().clone().requires_grad_(True) for k, v in P.items()}
    p1, p2 = fwd(leaves)
    val = MR.loss_on_p(p1, p2, batch["domain_id"], LW.KINDS[loss], sel)
    names = list(leaves)
    gs = torch.autograd.grad(val, [leaves[n] for n in names], allow_unused=True)
    return float(val.detach()), {n: (g if g is not None else torch.zeros_like(leaves[n])) for n, g in zip(names, gs)}


def check_sel(pl, B):
    sel = pl.sel.cpu().long()
    assert tuple(sel.shape) == (B, H) and bool((sel >= 1).all()) and bool((sel <= K).all()) and bool((sel[:, 1:] > sel[:, :-1]).all()), sel
    assert torch.equal(sel, MR.select(pl.z.cpu(), H, S)), "pl.sel against the rule on pl.z"
    return sel


def only_unkept_rows(batch, sel):
    """Table rows that the batch uses as candidates that were not kept and nowhere else."""
    B = sel.shape[0]
    keep = MR.kept_mask(sel, 1 + K)[:, 1:]
    neg = batch["neg_samples"].reshape(B, K).long()
    used = set(batch["i_node"].reshape(-1).tolist()) | set(batch["seq_d1"].reshape(-1).tolist()) | set(batch["seq_d2"].reshape(-1).tolist())
    used |= set(neg[keep].tolist())
    return sorted(set(neg[~keep].tolist()) - used)


@pytest.mark.parametrize("loss", ["softmax", "bpr"])
@pytest.mark.parametrize("model", MODELS)
def test_mined_gradients_against_the_float64_oracle(model, loss):
    B = 32 if model == "sasrec_itc" else 8
    P, batch, fwd, _, loss_tol, tol = SETUPS[model](B, T, 128, K, model == "sasrec_itc")
    eng = make_engine(model, P, B, loss, hard_negs=H, hard_skip=S)
    pl = run_engine(eng, batch)
    sel = check_sel(pl, B)
    want, grads = mined_oracle(P, fwd, batch, loss, sel)
    own, ar = (batch["domain_id"] != 0).long(), torch.arange(B)
    dz = torch.stack((pl.dp1.cpu(), pl.dp2.cpu()))
    assert torch.equal(dz[1 - own, ar], torch.zeros(B, 1 + K))
    keep = MR.kept_mask(sel, 1 + K)
    assert torch.equal(dz[own, ar][~keep], torch.zeros(int((~keep).sum())))
    rows = only_unkept_rows(batch, sel)
    assert rows, "the batch has no row that is a non-kept candidate only"
    from tests.test_gpu_sasrec import dense_table_grad
    assert torch.equal(dense_table_grad(eng, pl)[rows], torch.zeros(len(rows), 128)) and float(grads[TABLE][rows].abs().max()) == 0.0
    compare(f"mined {model} {loss} T {T} K {K} H {H} S {S}", eng, pl, want, grads, loss_tol, tol, True)


def train_masks(model, eng, B):
    if model in ("sasrec", "sasrec_itc"):
        return orc.philox_masks_sasrec(B, T, 128, seed=eng.seed, step=1)
    if model == "bert4rec":
        return orc.philox_masks_bert4rec(B, T, seed=eng.seed, step=1)
    return None


def train_forward(model, batch, masks, B):
    args = (batch["i_node"], batch["neg_samples"], batch["seq_d1"], batch["seq_d2"])
    if model in ("sasrec", "sasrec_itc"):
        kw = dict(isItC=True, threshold2=0.03) if model == "sasrec_itc" else {}
        return lambda L_, taps=None: orc.sasrec_forward(L_, *args, masks, taps, **kw)
    if model == "bert4rec":
        return lambda L_, taps=None: orc.bert4rec_forward(L_, *args, masks)
    return lambda L_, taps=None: gru_ref.gru4rec_forward(L_, *args)


@pytest.mark.parametrize("loss", ["softmax", "bpr"])
@pytest.mark.parametrize("model", MODELS)
def test_one_mined_train_step_against_dense_adam(model, loss):
    B = 32 if model == "sasrec_itc" else 8
    P, batch, _, _, _, _ = SETUPS[model](B, T, 128, K, model == "sasrec_itc")
    P64 = {k: v.double() for k, v in P.items()}
    for seed in range(3, 12):                   # isItC: a dropout seed under which the gate keeps its softmax margin in float64
        eng = make_engine(model, P, B, loss, seed=seed, hard_negs=H, hard_skip=S)
        masks = train_masks(model, eng, B)
        fwd = train_forward(model, batch, masks, B)
        if model != "sasrec_itc":
            break
        taps = {}
        with torch.no_grad():
            fwd(P64, taps)
        if 0 < int(taps["itc_d1"]["gate"].sum()) < B and taps["itc_d1"]["margin"] > 1e-3:
            break
    else:
        raise AssertionError("no dropout seed keeps the gate's margin")
    pl = eng.plan(B, T, 1 + K, need_grad=True)
    cu = {k: v.cuda() for k, v in batch.items()}
    eng.load_batch(pl, cu["i_node"], cu["neg_samples"], cu["seq_d1"], cu["seq_d2"], cu["label"], cu["domain_id"])
    eng.enqueue_train_step(pl)
    eng.flush_table()
    eng.sync()
    eng.check_index_error(pl)
    sel = check_sel(pl, B)
    want, grads = mined_oracle(P, fwd, batch, loss, sel)
    Po = {k: v.double().clone() for k, v in P.items()}
    orc.DenseAdam(Po, lr=1e-3).step(Po, grads)
    got = float(pl.loss.item())
    tag = f"mined step {model} {loss}"
    print(f"{tag}: loss {got:.7f} oracle {want:.7f}")
    log(f"{tag}: loss {got:.7f} oracle {want:.7f}")
    assert abs(got - want) < 5e-5 * max(1.0, abs(want)), (got, want)
    sd = {k: v.detach().cpu() for k, v in eng.state_dict().items()}
    bad = []
    for k, v in Po.items():
        if k == TABLE:
            continue
        d = (sd[k].double() - v).abs()
        if k.endswith("in_proj_bias"):                      # the key bias: its true gradient is zero (tests/test_gpu_optim.py check_params)
            n = v.numel() // 3
            d = torch.cat((d[:n], d[2 * n:]))
        if k.endswith("linear_layers.1.bias"):
            continue
        if k == "predictModule.fc.2.bias":                  # no gradient from a listwise objective: Adam's bound on a step only
            assert float((sd[k].double() - P64[k]).abs().max()) <= 1e-3 * (1 + 1e-6), k
            continue
        print(f"{tag} {k:50s} max |diff| {float(d.max()):.3e}")
        if not float(d.max()) < 1e-4:
            bad.append((k, float(d.max())))
    rel = float((sd[TABLE].double() - Po[TABLE]).abs().max() / Po[TABLE].abs().max())
    print(f"{tag} table relmax {rel:.3e}")
    log(f"{tag} table relmax {rel:.3e}")
    if not rel < 1e-5:
        bad.append((TABLE, rel))
    assert not bad, (tag, bad)
    # the candidates that were not kept: in the step's index list, zero gradient -- the row and its moments as dense Adam leaves them
    rows = only_unkept_rows(batch, sel)
    assert rows
    ids = pl.uniq_ids[:int(pl.n_uniq.item())].cpu().long().tolist()
    assert set(rows) <= set(ids), "a non-kept candidate left the step's index list"
    assert torch.equal(sd[TABLE][rows], P[TABLE][rows])
    assert torch.equal(eng.table_m[rows].cpu(), torch.zeros(len(rows), 128)) and torch.equal(eng.table_v[rows].cpu(), torch.zeros(len(rows), 128))


@pytest.mark.parametrize("kind,loss", [("sasrec", "softmax"), ("sasrec_itc", "bpr"), ("bert4rec", "bpr"), ("gru4rec", "softmax")])
def test_pooled_two_step_graph_equals_eager_steps(kind, loss):
    """Four train steps, dropout on: two replays of a 2-step graph over the input pool against four eager pool steps."""
    B, T_, n = (32 if kind == "sasrec_itc" else 8), 20, 4
    ep = epoch(n, B, T_, K, seed=31)
    out = []
    for graph in (True, False):
        m = make_model(kind, B, T_, loss=loss, hard_negs=H, hard_skip=S)
        m.train()
        m.begin_epoch_pool(ep)
        losses = []
        for _ in range(n // 2 if graph else n):
            v = m.pool_step(n_steps=2) if graph else m.pool_step(use_graph=False)
            m.engine.sync()
            losses.append(float(v.item()))
        m.end_epoch_pool()
        pl = m._last_plan
        out.append((losses, flushed(m), pl.sel.cpu().clone(), pl.z.cpu().clone()))
    (lg, sg, selg, zg), (le, se, sele, ze) = out
    assert all(map(lambda x: x == x and abs(x) < 1e3, lg + le)), (lg, le)
    assert lg == le[1::2], (lg, le)
    assert all(torch.equal(sg[k], se[k]) for k in sg), [k for k in sg if not torch.equal(sg[k], se[k])]
    assert torch.equal(selg, sele) and torch.equal(zg, ze)


@pytest.mark.parametrize("loss", ["softmax", "bpr"])
def test_hard_negs_zero_is_the_listwise_model(loss):
    """SASRec(..., loss=) without the keywords and with hard_negs = 0, hard_skip = 0: the same parameters after three steps."""
    B, T_ = 8, 20
    ep = epoch(3, B, T_, K, seed=32)
    sd = []
    for kw in ({}, {"hard_negs": 0, "hard_skip": 0}):
        m = make_model("sasrec", B, T_, loss=loss, **kw)
        m.train()
        for i in range(3):
            m.train_step(ep["i_node"][i], ep["neg_samples"][i], ep["seq_d1"][i], ep["seq_d2"][i], ep["label"], ep["domain_id"][i])
        assert not hasattr(m._last_plan, "sel")
        sd.append(flushed(m))
    assert all(torch.equal(sd[0][k], sd[1][k]) for k in sd[0])


def test_mining_changes_the_step_and_all_kept_does_not():
    """H = K, S = 0 trains as the listwise model does (the same list); H < K does not."""
    B, T_ = 8, 20
    ep = epoch(2, B, T_, K, seed=33)
    sd = []
    for kw in ({}, {"hard_negs": K}, {"hard_negs": H, "hard_skip": S}):
        m = make_model("sasrec", B, T_, loss="softmax", **kw)
        m.train()
        ls = []
        for i in range(2):
            v = m.train_step(ep["i_node"][i], ep["neg_samples"][i], ep["seq_d1"][i], ep["seq_d2"][i], ep["label"], ep["domain_id"][i])
            m.engine.sync()
            ls.append(float(v.item()))
        sd.append((ls, flushed(m)))
    assert sd[0][0][0] == sd[1][0][0], (sd[0][0], sd[1][0])                # the first loss: the listwise launch's bits
    assert sd[2][0][0] < sd[0][0][0] and math.isfinite(sd[2][0][1])        # fewer terms under the logsumexp
    assert any(not torch.equal(sd[0][1][k], sd[2][1][k]) for k in sd[0][1])


# ---------------------------------------------------------------------------- refusals
def test_refusals():
    from amid_amd.engine import SasrecEngine
    from amid_amd.engine_bert import Bert4recEngine
    from amid_amd.engine_gru import Gru4recEngine
    from amid_amd.model_seq import SASRec
    for cls in (SasrecEngine, Bert4recEngine, Gru4recEngine):
        with pytest.raises(ValueError, match="hard_negs"):
            cls(N_ITEMS, 128, 20, HID, hard_negs=2)
        with pytest.raises(ValueError, match="hard_negs"):
            cls(N_ITEMS, 128, 20, HID, loss="softmax", hard_negs=-1)
        with pytest.raises(ValueError, match="hard_skip"):
            cls(N_ITEMS, 128, 20, HID, loss="bpr", hard_skip=1)
    with pytest.raises(ValueError, match="isDR"):
        SasrecEngine(N_ITEMS, 128, 20, HID, dr=True, loss="softmax", hard_negs=2)
    with pytest.raises(ValueError, match="bf16"):
        SasrecEngine(N_ITEMS, 128, 20, HID, compute="bf16", loss="bpr", hard_negs=2)
    with pytest.raises(ValueError, match="isInC"):
        SasrecEngine(N_ITEMS, 128, 20, HID, inc_bs=8, loss="softmax", hard_negs=2)
    with pytest.raises(ValueError, match="isItC"):
        Gru4recEngine(N_ITEMS, 128, 20, HID, itc_bs=8, loss="softmax", hard_negs=2)
    with pytest.raises(ValueError, match="hard_negs"):
        SASRec(10, 128, N_ITEMS, 128, 20, HID, 8, False, False, 0.5, 0.5, hard_negs=2)
    # the first step: more than the row's negatives
    P, batch, _, _, _, _ = SETUPS["sasrec"](8, T, 128, 4, False)
    eng = make_engine("sasrec", P, 8, "softmax", hard_negs=4, hard_skip=1)
    with pytest.raises(ValueError, match="exceeds the 4 negatives"):
        run_engine(eng, batch)
    eng.sync()

    class World2:                                # an exchange over two ranks: refused before anything is exchanged
        world, active, grad_scale = 2, True, 0.5
    eng = SasrecEngine(N_ITEMS, 128, 20, HID, loss="softmax", hard_negs=2)
    pl = eng.plan(8, 20, 5, need_grad=True)
    with pytest.raises(ValueError, match="data-parallel"):
        eng.train_step_dp(pl, World2())


# ---------------------------------------------------------------------------- the command line, in a fresh process
def test_cli_trains_with_the_flags_and_logs_the_logit_means(tmp_path):
    from tests.test_gpu_checkpoint import _cli, _data, _log
    base = _data(tmp_path, False) + ["--seeds", "1", "--epoch", "1", "--max_steps", "2", "--train_negs", str(K), "--loss", "softmax",
                                     "--hard_negs", str(H), "--hard_skip", str(S)]
    logs = tmp_path / "logs"
    _cli("amid_amd.train_sr", base + ["-md", str(logs)])
    lines = _log(logs / "log0.txt")
    assert any(f"'hard_negs': {H}" in ln and f"'hard_skip': {S}" in ln for ln in lines)
    hits = [re.search(r"hard negatives, last step: mean logit kept ([-+0-9.eE]+|nan|inf) \tnot kept ([-+0-9.eE]+|nan|inf)", ln) for ln in lines]
    hits = [h for h in hits if h]
    assert len(hits) == 1, lines[-20:]
    kept, other = float(hits[0].group(1)), float(hits[0].group(2))
    assert math.isfinite(kept) and math.isfinite(other), (kept, other)
