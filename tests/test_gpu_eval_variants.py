"""The fused evaluation batch (SasrecEngine.enqueue_eval / eval_epoch, SASRec.eval_ranks) for the isDR, isItC and isInC models and their
combinations: bit for bit against the launches it replaces (enqueue_forward over both domains with the candidates' rows gathered by K1 +
amid_positive_rank_f32), against the oracle at the bar the same model's forward is held to in tests/test_gpu_sasrec.py, through the captured
graph, through train_sr.test(), and downstream in full_ranks / recommend."""
import argparse
import json

import numpy as np
import pytest
import torch

from oracle import amid_oracle as orc

pytestmark = pytest.mark.gpu
FIX = 1e-7
VARIANTS = {"dr": dict(dr=True), "itc": dict(itc=True), "itc+dr": dict(itc=True, dr=True), "inc": dict(inc=True), "inc+dr": dict(inc=True, dr=True)}


def shapes_of(variant, n_items, D, T, hid, B):
    v = VARIANTS[variant]
    return orc.sasrec_param_shapes(n_items, D, T, hid, itc_bs=B if v.get("itc") else 0, dr=bool(v.get("dr")), inc_bs=B if v.get("inc") else 0)


def make_engine(variant, P, n_items, D, T, hid, B, ts1=0.5, ts2=0.5, compute="f32"):
    from amid_amd.engine import SasrecEngine
    v = VARIANTS[variant]
    kw = {}
    if v.get("itc"):
        kw.update(itc_bs=B, itc_threshold=ts2)
    if v.get("inc"):
        kw.update(inc_bs=B, inc_threshold=ts1)
    if v.get("dr"):
        kw.update(dr=True)
    eng = SasrecEngine(n_items, D, T, hid, device="cuda:0", lr=1e-3, seed=5, compute=compute, **kw)
    eng.load_state_dict(P)
    return eng


def eval_batch(B, T, n_items, NI, seed, dup_positive=False):
    b = orc.synthetic_batch(B, T, n_items - 1, pad_id=n_items - 1, neg=NI - 1, seed=seed)
    if dup_positive:                    # the positive's own id among the negatives: an exact tie, counted against the positive only with fix_value
        b["neg_samples"][::2, 3] = b["i_node"][::2]
    b["label"] = torch.zeros(B, NI)
    b["label"][:, 0] = 1.0
    return b


def old_path(eng, pl, cu):
    """What test() ran for these models before: the eval forward over every sequence with the candidates gathered by K1 (isDR: three scorers
    over them), then the rank kernel."""
    from amid_amd.utils import device_positive_ranks
    eng.load_batch(pl, cu["i_node"], cu["neg_samples"], cu["seq_d1"], cu["seq_d2"], cu["label"], cu["domain_id"])
    eng.enqueue_prepare(pl, sparse=False)
    eng.enqueue_forward(pl, train=False, with_loss=False)
    eng.sync()
    torch.cuda.current_stream().wait_stream(eng.stream)
    p1, p2 = pl.p1.clone(), pl.p2.clone()
    r = device_positive_ranks(p1, p2, cu["domain_id"], FIX)
    r0 = device_positive_ranks(p1, p2, cu["domain_id"], 0.0)
    torch.cuda.synchronize()
    own = torch.where(cu["domain_id"][:, None] != 0, p2, p1)
    u_own = torch.where(cu["domain_id"][:, None] != 0, pl.u[1], pl.u[0]).clone()
    return own, r, r0, u_own


def loss_close(got, own, y, B, NI):
    want = torch.nn.functional.binary_cross_entropy(own.double(), y.double(), reduction="none").sum(1) / (B * NI)      # train_sr.py:63-64
    err, bar = float((got.double() - want).abs().max()), 1e-6 * float(want.abs().max()) + 1e-9
    print(f"loss_part err {err:.3e} bar {bar:.3e}")
    return err <= bar


RUNSH = (128, 32, 20, 256, 1000, "f32")          # run.sh: mybank, T 20, B 256, D 128, hid 32, 999 negatives
CASES = [(v, *s) for v in VARIANTS for s in (RUNSH, (128, 32, 33, 7, 5, "f32"), (64, 16, 20, 16, 100, "f32"))]
CASES.append(("itc+dr", 128, 32, 50, 24, 100, "bf16"))
# more batches of the sizes InterComp's mix takes its 512-thread form on (32 .. 256 rows): D 64, the general scorer at D 128, an odd batch
CASES += [("itc", 64, 16, 20, 48, 100, "f32"), ("itc+dr", 128, 64, 20, 40, 130, "f32"), ("itc", 128, 32, 20, 33, 70, "f32"), ("itc", 64, 32, 50, 255, 9, "f32")]


@pytest.mark.parametrize("variant,D,hid,T,B,NI,compute", CASES)
def test_eval_launches_are_bit_identical_to_the_forward_and_rank_kernels(variant, D, hid, T, B, NI, compute):
    n_items = 3000
    P = orc.random_params(shapes_of(variant, n_items, D, T, hid, B), seed=3 + D + T)
    # a threshold near the batch softmax's mean: gates of both kinds whenever the softmax is not one-hot (either way both paths run the
    # same module on the same inputs)
    eng = make_engine(variant, P, n_items, D, T, hid, B, ts1=1.0 / B, ts2=1.0 / B, compute=compute)
    pl = eng.plan(B, T, NI, need_grad=False)
    assert eng.eval_fused_ok(pl)
    for seed in range(3):
        cu = {k: v.cuda() for k, v in eval_batch(B, T, n_items, NI, 40 + seed, dup_positive=NI > 4).items()}
        torch.cuda.synchronize()          # (the engine's stream does not wait for torch's)
        own, r, r0, u_own = old_path(eng, pl, cu)
        pl.p1.zero_(); pl.p2.zero_()
        torch.cuda.synchronize()
        eng.load_batch(pl, cu["i_node"], cu["neg_samples"], cu["seq_d1"], cu["seq_d2"], cu["label"], cu["domain_id"])
        eng.enqueue_eval(pl, FIX, with_loss=True, want_scores=True)
        eng.sync()
        eng.check_index_error(pl)
        print(f"{variant} seed {seed}: max |ev_p - own| {float((pl.ev_p - own).abs().max()):.3e}, max |ev_u - u| {float((pl.ev_u - u_own).abs().max()):.3e}, "
              f"rank diffs {int((pl.ev_rank != r).sum())} raw {int((pl.ev_rank_raw != r0).sum())}")
        assert torch.equal(pl.ev_u, u_own)
        assert torch.equal(pl.ev_p, own), float((pl.ev_p - own).abs().max())
        assert torch.equal(pl.ev_rank, r) and torch.equal(pl.ev_rank_raw, r0)
        if NI > 4:                      # the tie rule: a row whose positive repeats among the negatives loses (at least) one more rank with fix_value
            assert bool((pl.ev_rank[::2] >= pl.ev_rank_raw[::2] + 1).all()) and bool((pl.ev_rank >= pl.ev_rank_raw).all())
            ties = (own[:, 1:] == own[:, :1]).sum(1).int()
            assert bool((pl.ev_rank - pl.ev_rank_raw >= ties).all())
        assert loss_close(pl.ev_loss_part, own, cu["label"], B, NI)
        # no copy of the candidates' rows, no scores of the other domain: the new path leaves the forward's outputs alone
        assert not bool(pl.p1.any()) and not bool(pl.p2.any())


# ---------------------------------------------------------------------------- against the oracle
def pick_threshold(softmaxes):
    """Midway across the widest gap of the oracle's batch-softmax values that leaves every module a gate with at least one 1 and one 0
    (two modules share one threshold: the gap is the smaller of their two around the candidate)."""
    vals = torch.cat([s.double().reshape(-1) for s in softmaxes]).sort().values
    best, best_t = -1.0, None
    for t in ((vals[1:] + vals[:-1]) / 2).tolist():
        if all(0 < int((s > t).sum()) < s.numel() for s in softmaxes):
            m = min(float((s.double() - t).abs().min()) for s in softmaxes)
            if m > best:
                best, best_t = m, t
    assert best_t is not None
    return float(best_t)


def oracle_case(variant, D, hid, T, B, NI, n_items, seed):
    """CPU: parameters, a batch, thresholds chosen from the oracle's own softmax values, the oracle's own-domain scores.  Asserts the
    conditions of tests/test_gpu_sasrec.py on the inputs: every comp module's gate has a 1 and a 0, and its softmax keeps > 1e-3 from the
    threshold."""
    v = VARIANTS[variant]
    P = orc.random_params(shapes_of(variant, n_items, D, T, hid, B), seed=seed)
    if v.get("itc"):
        for d in (1, 2):
            P[f"sac{d}.last_layernorm.weight"] *= 0.3 if B <= 8 else 0.5      # keeps the batch softmax of the pair-max scores away from one-hot
    if v.get("inc"):                                                         # (and, over 256 rows, its largest values more than 2e-3 apart)
        P["item_emb_layer.emb_item.weight"] *= 0.35        # self pair-max scores about a unit apart: a softmax neither flat nor one-hot
    g = torch.Generator().manual_seed(seed + 1)
    b = eval_batch(B, T, n_items, NI, seed + 2)
    b["seq_d1"] = torch.randint(1, n_items - 1, (B, T), generator=g)      # no shared pad positions: distinct pair-max scores
    b["seq_d2"] = torch.randint(1, n_items - 1, (B, T), generator=g)
    kw = dict(isItC=bool(v.get("itc")), isInC=bool(v.get("inc")), isDR=bool(v.get("dr")))
    ts1 = ts2 = 0.5
    taps = {}
    with torch.no_grad():
        if v.get("itc") or v.get("inc"):          # the softmax values do not depend on the threshold
            orc.sasrec_forward(P, b["i_node"], b["neg_samples"][:, :1], b["seq_d1"], b["seq_d2"], None, taps, **kw)
            if v.get("itc"):
                ts2 = pick_threshold([taps["itc_d1"]["softmax"], taps["itc_d2"]["softmax"]])
            if v.get("inc"):
                ts1 = pick_threshold([taps["inc_d1"]["softmax"], taps["inc_d2"]["softmax"]])
        taps = {}
        outs = orc.sasrec_forward(P, b["i_node"], b["neg_samples"], b["seq_d1"], b["seq_d2"], None, taps, threshold1=ts1, threshold2=ts2, **kw)
    for pre in (["itc_d1", "itc_d2"] if v.get("itc") else []) + (["inc_d1", "inc_d2"] if v.get("inc") else []):
        gate = taps[pre]["gate"]
        print(f"{variant} {pre}: threshold {ts2 if pre.startswith('itc') else ts1:.6f} gate ones {int(gate.sum())} / {B} margin {taps[pre]['margin']:.3e}")
        assert 0 < int(gate.sum()) < B and taps[pre]["margin"] > 1e-3
    want = torch.where(b["domain_id"][:, None] != 0, outs[1].reshape(B, -1), outs[0].reshape(B, -1))
    return P, b, ts1, ts2, want, taps


ORACLE_CASES = [(v, D, hid, 20, 8, 50) for v in VARIANTS for D, hid in ((64, 16), (128, 32))] + [("itc+dr", *RUNSH[:5])]


@pytest.mark.parametrize("variant,D,hid,T,B,NI", ORACLE_CASES)
def test_eval_scores_against_the_oracle(variant, D, hid, T, B, NI):
    """pl.ev_p against the oracle's eval-mode forward of the same model (CPU restatement of model_seq.py:416-443), at the bar that model's
    forward is held to in tests/test_gpu_sasrec.py: relmax < 3e-5 (isItC :368, isInC :449, isInC + isItC (+ isDR) :520; isDR has no looser one
    of its own there)."""
    n_items = 300 if B == 8 else 3000
    P, b, ts1, ts2, want, taps = oracle_case(variant, D, hid, T, B, NI, n_items, seed=60 + D)
    eng = make_engine(variant, P, n_items, D, T, hid, B, ts1, ts2)
    pl = eng.plan(B, T, NI, need_grad=False)
    assert eng.eval_fused_ok(pl)
    cu = {k: v.cuda() for k, v in b.items()}
    torch.cuda.synchronize()
    eng.load_batch(pl, cu["i_node"], cu["neg_samples"], cu["seq_d1"], cu["seq_d2"], cu["label"], cu["domain_id"])
    eng.enqueue_eval(pl, FIX, want_scores=True)
    eng.sync()
    eng.check_index_error(pl)
    v = VARIANTS[variant]
    if v.get("itc"):
        assert torch.equal(pl.itc_gate.cpu(), taps["itc_d1"]["gate"])
    if v.get("inc"):
        for d in (1, 2):
            assert torch.equal(pl.inc_gate[d - 1].cpu(), taps[f"inc_d{d}"]["gate"])
    got = pl.ev_p.cpu().double()
    e = float((got - want.double()).abs().max() / (want.double().abs().max() + 1e-30))
    print(f"{variant} D {D} B {B}: relmax {e:.3e}")
    assert e < 3e-5


# ---------------------------------------------------------------------------- graph and epoch
def test_eval_epoch_graph_equals_eager_and_the_old_path_at_the_shipped_command_lines_shape():
    """isItC + isDR at run.sh's shape over 8 batches: eval_epoch through the captured graph = without it = the launches it replaces.  The
    images come from pack_epoch (an isDR plan's image ends in B ob_label words)."""
    D, hid, T, B, NI, _ = RUNSH
    n_items, nb = 20000, 8
    P = orc.random_params(shapes_of("itc+dr", n_items, D, T, hid, B), seed=77)
    eng = make_engine("itc+dr", P, n_items, D, T, hid, B, ts2=1.0 / B)
    pl = eng.plan(B, T, NI, need_grad=False)
    assert eng.eval_fused_ok(pl)
    cus = [{k: v.cuda() for k, v in eval_batch(B, T, n_items, NI, 900 + i).items()} for i in range(nb)]
    torch.cuda.synchronize()
    st = lambda k: torch.stack([c[k] for c in cus])      # noqa: E731
    packed = eng.pack_epoch(pl, st("i_node"), st("neg_samples"), st("seq_d1"), st("seq_d2"), cus[0]["label"], st("domain_id"))
    assert packed.shape == (nb, pl.in_words)
    torch.cuda.synchronize()
    out_g = eng.eval_epoch(pl, packed, FIX, with_loss=True, use_graph=True)
    eng.sync()
    assert (FIX, True) in pl.eval_graphs
    out_e = eng.eval_epoch(pl, packed, FIX, with_loss=True, use_graph=False)
    eng.sync()
    assert torch.equal(out_g, out_e)
    for i, c in enumerate(cus):
        own, r, r0, _ = old_path(eng, pl, c)
        assert torch.equal(out_g[i, :B], r) and torch.equal(out_g[i, B:2 * B], r0), i
        assert loss_close(out_g[i, 2 * B:].view(torch.float32), own, c["label"], B, NI)


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


@pytest.mark.parametrize("kind,emb,overlap", [("itc+dr", 128, True), ("inc", 64, False), ("itc+dr", 64, False), ("inc", 128, False)])
def test_train_sr_test_gives_the_same_metrics_either_way(tmp_path, kind, emb, overlap):
    """train_sr.test() through SASRec.eval_ranks and through model.forward + BCE + the rank kernel on the same evaluation set and negatives:
    the same metrics exactly, the same loss to rounding."""
    from amid_amd import model_seq
    from amid_amd.dataset_seq import DeviceBatches, DualDomainSeqDataset
    from amid_amd.train_sr import test
    rng = np.random.default_rng(5)
    _write_csv(tmp_path / "toy_test.csv", 192, rng, 1, 400, 400, 900)
    ds = DualDomainSeqDataset(seq_len=20, isTrain=False, neg_nums=99, long_length=7, pad_id=1001, seed=3, csv_path=str(tmp_path / "toy_test.csv"))
    v = VARIANTS[kind]
    model = model_seq.SASRec(10, emb, 1100, emb, 20, 32, 32, bool(v.get("inc")), bool(v.get("itc")), 0.03, 0.03, isDR=bool(v.get("dr")), seed=2)
    args = argparse.Namespace(overlap=overlap)
    res = {}
    for fused in (True, False):
        model.engine.EVAL_FUSED = fused
        vb = DeviceBatches(ds, 32, shuffle=False, device="cuda:0", seed=9)
        ep = vb.epoch_tensors()
        assert (model.eval_ranks(ep, FIX) is not None) == fused
        vb = DeviceBatches(ds, 32, shuffle=False, device="cuda:0", seed=9)
        res[fused] = test(model, args, vb)
    assert set(res[True]) == set(res[False])
    for k, val in res[False].items():
        if k == "loss":
            print(f"{kind}: loss fused {res[True][k]!r} forward {val!r}")
            assert abs(res[True][k] - val) <= 1e-6 * abs(val)
        else:
            assert res[True][k] == val or all(np.isnan(a) and np.isnan(b) or a == b for a, b in zip(res[True][k], val)), k


# ---------------------------------------------------------------------------- downstream
def test_full_ranks_and_recommend_of_an_itc_model_do_not_depend_on_the_switch(tmp_path):
    """full_ranks and recommend take their user vectors from enqueue_user_vectors: pl.ev_u (the MIXED vector, stride 0) with the fused
    evaluation, enqueue_forward's pl.u without -- the same ranks, ids and scores, bitwise."""
    from amid_amd import model_seq
    from amid_amd.dataset_seq import DeviceBatches, DualDomainSeqDataset
    rng = np.random.default_rng(8)
    _write_csv(tmp_path / "toy_test.csv", 128, rng, 1, 60, 60, 119)
    ds = DualDomainSeqDataset(seq_len=20, isTrain=False, neg_nums=30, long_length=7, pad_id=119, seed=3, csv_path=str(tmp_path / "toy_test.csv"))
    bs = 32
    model = model_seq.SASRec(10, 64, 120, 64, 20, 16, bs, False, True, 0.5, 0.03, seed=2)
    model.eval()
    g = torch.Generator().manual_seed(2)
    s1 = torch.randint(1, 60, (bs, 20), generator=g)
    s2 = torch.randint(60, 119, (bs, 20), generator=g)
    dom = torch.randint(0, 2, (bs,), generator=g)
    res = {}
    for fused in (True, False):
        model.engine.EVAL_FUSED = fused
        vb = DeviceBatches(ds, bs, shuffle=False, device="cuda:0", seed=9)
        ep = vb.epoch_tensors()
        pl = model.engine.plan(bs, 20, 31, need_grad=False)
        assert model.engine.eval_fused_ok(pl) == fused
        fr = model.full_ranks(ep, vb, FIX)
        ids, scores = model.recommend(s1, s2, dom, k=10)
        torch.cuda.synchronize()
        res[fused] = (fr["rank"].clone(), fr["rank_raw"].clone(), ids.clone(), scores.clone())
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)
    assert int(res[True][0].max()) > 0
