"""tests/comp_ref.py (the reference of tests/test_gpu_innercomp.py) in float64 against oracle.amid_oracle.inter_comp / inner_comp and their
autograd -- which tests/test_oracle_golden.py g9, g12, g14 and g15 pin to the reference's own outputs --, its two summation orders against
each other, and the mutants of a kernel against the bar of the GPU test at every shape of that test.  None of it needs a GPU."""
import pytest
import torch

from oracle import amid_oracle as orc
from tests import comp_ref as R

F64 = torch.float64
SHAPES = [(5, 4, 8), (9, 7, 12)]                                  # (B, T, D)
TOL = 1e-12


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def small_case(cross, B, T, D):
    g = torch.Generator().manual_seed(100 * B + 10 * T + D + cross)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)      # noqa: E731
    x = rn(2, B, T, D) * (0.3 + 0.3 * torch.rand(2, B, 1, 1, generator=g, dtype=F64))
    P = dict(wnn=rn(2, D, D) / D ** 0.5, bnn=0.3 * rn(2, D), wbs=rn(2, B) / B ** 0.5, bbs=rn(2, 1))
    dx0 = rn(2, B, 2 * T, D)
    s = R.scores(x, cross)
    thr, gate, margin, _ = R.pick_gate(s, [s])
    assert margin > 1e-6
    return x, P, dx0, thr, gate


@pytest.mark.parametrize("B,T,D", SHAPES)
@pytest.mark.parametrize("cross", [0, 1])
def test_float64_restatement_is_the_oracle(cross, B, T, D):
    x, P, dx0, thr, gate = small_case(cross, B, T, D)
    r = R.forward(x, P, cross, F64, threshold=thr)
    assert torch.equal(r["gate"], gate.to(F64))
    r.update(R.backward(x, P, cross, F64, r["gate"], dx0))
    oP = {}
    for g in (0, 1):
        oP.update({f"m{g}.trans_nn.weight": P["wnn"][g], f"m{g}.trans_nn.bias": P["bnn"][g], f"m{g}.trans_bs.weight": P["wbs"][g][None],
                   f"m{g}.trans_bs.bias": P["bbs"][g]})
    oP = {k: v.clone().requires_grad_(True) for k, v in oP.items()}
    xl = x.clone().requires_grad_(True)
    taps, out = {}, []
    for g in (0, 1):
        out.append(orc.inter_comp(xl[g], xl[1 - g], oP, f"m{g}", thr, taps) if cross else orc.inner_comp(xl[g], oP, f"m{g}", thr, taps))
    out = torch.stack(out)
    (out * dx0).sum().backward()
    want = dict(s=torch.stack([taps[f"m{g}"]["s"] for g in (0, 1)]), softmax=torch.stack([taps[f"m{g}"]["softmax"] for g in (0, 1)]),
                gate=torch.stack([taps[f"m{g}"]["gate"] for g in (0, 1)]), x0=out.detach(), Z=out.detach()[:, 0, T:], dxg=xl.grad,
                dw_nn=torch.stack([oP[f"m{g}.trans_nn.weight"].grad for g in (0, 1)]),
                db_nn=torch.stack([oP[f"m{g}.trans_nn.bias"].grad for g in (0, 1)]),
                dw_bs=torch.stack([oP[f"m{g}.trans_bs.weight"].grad[0] for g in (0, 1)]),
                db_bs=torch.stack([oP[f"m{g}.trans_bs.bias"].grad[0] for g in (0, 1)]))
    assert torch.equal(out.detach()[:, :, T:], out.detach()[:, :1, T:].expand(-1, B, -1, -1))       # one token group for every row
    for k, w in want.items():
        assert rel(r[k], w) <= TOL, (k, rel(r[k], w))
    # what the oracle does not expose follows from what it does
    assert rel(r["dZ"], dx0[:, :, T:].sum(1)) <= TOL and rel(r["sw"], P["wbs"].sum(1)) <= TOL
    assert rel(r["rows"][..., 0], r["dZ"].sum(-1)) <= TOL and rel(r["rows"][..., 1], (r["dZ"] * P["bnn"][:, None]).sum(-1)) <= TOL
    assert rel(r["db_bs"], r["rows"][..., 0].sum(1)) <= TOL
    assert rel(r["Z"], r["S"] @ P["wnn"].transpose(1, 2) + P["bnn"][:, None] * r["sw"][:, None, None] + P["bbs"][:, None]) <= TOL
    assert rel(r["dS"], r["dZ"] @ P["wnn"]) <= TOL


@pytest.mark.parametrize("B,T,D", SHAPES)
@pytest.mark.parametrize("cross", [0, 1])
@pytest.mark.parametrize("parts", [0, 3])
def test_index_order_is_torch_order_in_float64(cross, B, T, D, parts):
    x, P, dx0, thr, gate = small_case(cross, B, T, D)
    pos = 0.1 * torch.randn(2, 2 * T, D, dtype=F64, generator=torch.Generator().manual_seed(3))
    dz_parts = torch.randn(parts, 2, T, D, dtype=F64, generator=torch.Generator().manual_seed(4)) if parts else None
    r = {}
    for order in ("torch", "index"):
        r[order] = R.forward(x, P, cross, F64, order, threshold=thr, pos=pos)
        r[order].update(R.backward(x, P, cross, F64, gate, dx0, order, dz_parts=dz_parts))
    assert set(r["torch"]) == set(r["index"]) == {"s", "softmax", "gate", "x0", "tmq", *R.TENSORS_FWD, *R.TENSORS_BWD}
    assert torch.equal(r["index"].pop("tmq"), r["torch"].pop("tmq"))
    for k, w in r["torch"].items():
        assert rel(r["index"][k], w) <= TOL, (k, rel(r["index"][k], w))
    if parts:
        assert rel(r["torch"]["dZ"], dz_parts.sum(0)) <= TOL


def test_tmq_bits_and_positional_rows():
    x, P, dx0, thr, gate = small_case(0, 5, 4, 8)
    pos = torch.ones(2, 8, 8, dtype=F64)
    x[1, 2, 3, 5] = -1.0
    r = R.forward(x, P, 0, F64, threshold=thr, pos=pos)
    assert torch.equal(r["x0"][:, :, :4], x + 1.0) and r["tmq"].shape == (2, 5, 8, 2)
    want = torch.zeros(2, 5, 8, 2, dtype=torch.uint8)
    want[1, 2, 3, 1] = 2                                         # feature 5 = 4 * 1 + 1
    assert torch.equal(r["tmq"], want)


# ---------------------------------------------------------------------------- the mutants, at the shapes of the GPU test
def gpu_shapes():
    return [(form, B, T, D, None, nsplit) for form, B, T, D, nsplit in R.CHAIN_CASES] + \
        [(form, Bg, T, D, sizes, 1) for form, Bg, T, D, sizes in R.SHARD_CASES]


@pytest.mark.parametrize("form,B,T,D,sizes,nsplit", gpu_shapes())
def test_mutants_move_the_outputs(form, B, T, D, sizes, nsplit):
    """Score over a < c only: not at T = 1 (the diagonal is the only pair) nor with cross = 1 (all T x T pairs, no diagonal to leave out);
    w_bs[j] for w_bs[j0 + j]: only with more than one shard; cross = 1 mixing the module's own domain: only with cross = 1."""
    applied = R.mutants_move_the_outputs(form, B, T, D, sizes, nsplit)
    want = {"bnn_once", "dwbs_no_b"} | ({"no_diag"} if (R.FORMS[form] == 0 and T > 1) else set()) | ({"shard_j0"} if sizes and len(sizes) > 1 else set()) | \
        ({"cross_own"} if R.FORMS[form] else set())
    assert set(applied) == want
    R.assert_inputs(R.ref_case(form, B, T, D, nsplit, sizes))


@pytest.mark.parametrize("cross", [0, 1])
def test_score_limits(cross):
    assert R.last_accepted_T(cross) == (154 if cross else 309)
    assert R.score_lds(cross, 150, 128) == (158400 if cross else 79200) and R.score_lds(cross, 150, 128) > 64 * 1024
    assert R.largest_batch() == 15232
