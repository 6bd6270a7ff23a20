"""tests/listwise_ref.py (the restatement the GPU tests of csrc/head_listwise.hip compare against) held to torch.autograd on
torch.logsumexp / softplus, the two objectives against each other at NI = 2, and the conditions on the GPU cases' inputs."""
import pytest
import torch
import torch.nn.functional as F

from tests import head_ref as R
from tests import listwise_ref as LW

F64, F32 = torch.float64, torch.float32
SHAPES = [(3, 2, 16, 8), (2, 5, 32, 16), (2, 65, 32, 16), (1, 130, 8, 64)]      # (B, NI, D, hid)
# the cases of tests/test_gpu_listwise.py
GPU_SHAPES = [(1, 2, 32, 4), (3, 2, 128, 32), (2, 5, 96, 24), (2, 64, 128, 32), (2, 65, 128, 32), (2, 130, 64, 16), (1, 1024, 128, 64)]


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def inputs(B, NI, D, hid):
    g = torch.Generator().manual_seed(7 * B + 13 * NI + D + hid)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)      # noqa: E731
    W = dict(w1=rn(hid, 2 * D) / (2 * D) ** 0.5, b1=0.1 * rn(hid), w2=rn(hid) / hid ** 0.5, b2=0.1 * rn(1))
    return rn(2, B, D), 0.7 * rn(B, NI, D), W, torch.arange(B) % 2


@pytest.mark.parametrize("kind", ["softmax", "bpr"])
@pytest.mark.parametrize("B,NI,D,hid", SHAPES)
def test_restatement_against_autograd(B, NI, D, hid, kind):
    u, items, W, domain_id = inputs(B, NI, D, hid)
    r = LW.launch(u, items, W, domain_id, LW.KINDS[kind], F64)
    lin1, lin2 = torch.nn.Linear(2 * D, hid).double(), torch.nn.Linear(hid, 1).double()
    with torch.no_grad():
        lin1.weight.copy_(W["w1"]); lin1.bias.copy_(W["b1"]); lin2.weight.copy_(W["w2"][None]); lin2.bias.copy_(W["b2"])
    ua, ia = u.clone().requires_grad_(True), items.clone().requires_grad_(True)
    cat = torch.cat((ua[:, :, None, :].expand(2, B, NI, D), ia[None].expand(2, B, NI, D)), dim=-1)
    za = lin2(torch.relu(lin1(cat))).squeeze(-1)
    za.retain_grad()
    zo = za[(domain_id != 0).long(), torch.arange(B)]
    per = torch.logsumexp(zo, 1) - zo[:, 0] if kind == "softmax" else F.softplus(zo[:, 1:] - zo[:, :1]).mean(1)
    per.mean().backward()
    o = hid * 2 * D
    got = dict(z=(r["z"], za.detach()), p=(r["p"], torch.sigmoid(za.detach())), loss_part=(r["loss_part"], per.detach() / B), dz=(r["dz"], za.grad),
               du=(r["du"], ua.grad), ditems=(r["ditems"], ia.grad), dW1=(r["sc_dW1"].sum(0).view(hid, 2 * D), lin1.weight.grad),
               db1=(r["sc_db1"].sum(0), lin1.bias.grad), dW2=(r["sc_dW2"].sum(0), lin2.weight.grad[0]), db2=(r["sc_db2"].sum(0), lin2.bias.grad))
    # db2 = sum of dz is 0 in exact arithmetic under both objectives (they do not change when every logit moves alike): what is left of it
    # is rounding, held against the size of its terms
    mine, theirs = got.pop("db2")
    assert float((mine - theirs).abs().max()) <= 1e-13 * float(r["dz"].abs().sum()) and float(mine.abs().max()) <= 1e-13 * float(r["dz"].abs().sum())
    bad = {k: rel(a, b) for k, (a, b) in got.items() if not rel(a, b) <= 1e-11}
    assert not bad, bad
    # the other domain takes no gradient, exactly
    oth = 1 - (domain_id != 0).long()
    assert torch.equal(r["dz"][oth, torch.arange(B)], torch.zeros(B, NI, dtype=F64))
    assert torch.equal(r["du"][oth, torch.arange(B)], torch.zeros(B, D, dtype=F64))
    assert o + 2 * hid + 1 == sum(r[k].shape[1] for k in ("sc_dW1", "sc_db1", "sc_dW2", "sc_db2"))
    # the objective on p = sigmoid(z) is the objective on z
    q = LW.objective_on_p(r["p"], domain_id, LW.KINDS[kind], F64)
    assert rel(q["loss_part"], r["loss_part"]) <= 1e-11 and rel(q["dz"], r["dz"]) <= 1e-11


@pytest.mark.parametrize("B,D,hid", [(3, 16, 8), (2, 32, 64)])
def test_softmax_and_bpr_agree_at_two_candidates(B, D, hid):
    """lse(z0, z1) - z0 = softplus(z1 - z0): the loss and every gradient agree to rounding."""
    u, items, W, domain_id = inputs(B, 2, D, hid)
    a, b = (LW.launch(u, items, W, domain_id, k, F64) for k in (LW.SOFTMAX, LW.BPR))
    bad = {k: rel(a[k], b[k]) for k in a if k != "sc_db2" and not rel(a[k], b[k]) <= 1e-13}
    assert not bad, bad
    a, b = (LW.launch(u, items, W, domain_id, k, F32) for k in (LW.SOFTMAX, LW.BPR))
    bad = {k: rel(a[k], b[k]) for k in a if k != "sc_db2" and not rel(a[k], b[k]) <= 1e-5}
    assert not bad, bad


def test_float32_restatement_is_float32_and_near_the_float64_one():
    u, items, W, domain_id = inputs(2, 65, 32, 16)
    for kind in (LW.SOFTMAX, LW.BPR):
        r64, r32 = (LW.launch(u, items, W, domain_id, kind, t) for t in (F64, F32))
        assert all(v.dtype == F32 for v in r32.values())
        assert all(rel(r32[k].double(), r64[k]) <= 1e-4 for k in r64 if k != "sc_db2")


def test_saturated_logits_stay_finite_in_float32():
    """b2 = +40: every p == 1.0f; the objectives read z, so nothing is divided by p (1 - p) = 0.  Equal logits: softmax loss = log NI."""
    B, NI, D, hid = 2, 65, 32, 16
    u, items, W, domain_id = inputs(B, NI, D, hid)
    W = dict(W, b2=torch.tensor([40.0], dtype=F64))
    for kind in (LW.SOFTMAX, LW.BPR):
        r = LW.launch(u, items, W, domain_id, kind, F32)
        assert bool((r["p"] == 1.0).all()) and all(bool(torch.isfinite(v).all()) for v in r.values())
        assert float(r["dz"].abs().max()) > 0
    W0 = dict(W, w2=torch.zeros(hid, dtype=F64))
    r = LW.launch(u, items, W0, domain_id, LW.SOFTMAX, F32)
    # (lse = 40 + log 65 carries an ulp of 2^-18 = 3.8e-6; the loss is a difference of two such numbers)
    assert abs(float(r["loss_part"].sum()) - float(torch.log(torch.tensor(float(NI))))) < 4 * 2.0 ** -18


def test_gpu_case_inputs_meet_their_conditions():
    from tests import test_gpu_head as G
    steps = []
    for B, NI, D, hid in GPU_SHAPES:
        for dom in ("mixed", 0, 1):
            c = LW.case(B, NI, D, hid, dom)
            assert G.relu_margin_ok(c["u"], c["items"], c["W"]) and G.in_range(R.scorer(c["u"], c["items"], c["W"], F64)[0]), (B, NI, D, hid)
            assert c["items"].dtype == F32 and c["u"].dtype == F32
            assert B == 1 or dom != "mixed" or set(c["domain_id"].tolist()) == {0, 1}
            steps.append(c["steps"])
    assert max(steps) <= LW.MAX_SEED_STEPS, steps
    c = LW.case(2, 65, 128, 32, "mixed", True)
    assert bool((R.scorer(c["u"], c["items"], c["W"], F32)[0] == 1.0).all())
    print("seed steps per case:", steps)
