"""tests/mined_ref.py (the reference of tests/test_gpu_mined.py) against torch.autograd on logsumexp / softplus over z.gather(topk indices),
its tie rule, its identity with tests/listwise_ref.py at H = M, S = 0, the window shift of S and the zero gradient of the rows not kept."""
import pytest
import torch

from tests import listwise_ref as LW
from tests import mined_ref as MR

F64 = torch.float64
CASES = [(3, 9, 32, 8, 3, 0), (3, 9, 32, 8, 3, 2), (2, 17, 64, 16, 1, 0), (2, 17, 64, 16, 16, 0), (2, 6, 32, 4, 2, 3)]


def _inputs(B, NI, D, hid, seed=0):
    g = torch.Generator().manual_seed(1000 * B + NI + seed)
    u = torch.randn(2, B, D, generator=g, dtype=F64)
    items = torch.randn(B, NI, D, generator=g, dtype=F64)
    W = dict(w1=torch.randn(hid, 2 * D, generator=g, dtype=F64) / D ** 0.5, b1=0.1 * torch.randn(hid, generator=g, dtype=F64),
             w2=torch.randn(hid, generator=g, dtype=F64) / hid ** 0.5, b2=0.1 * torch.randn(1, generator=g, dtype=F64))
    dom = torch.tensor([b % 2 for b in range(B)])
    return u, items, W, dom


def _autograd(u, items, W, dom, kind, H, S):
    """The mined loss with torch.topk's indices as constants, differentiated by autograd."""
    u, items = u.clone().requires_grad_(True), items.clone().requires_grad_(True)
    W = {k: v.clone().requires_grad_(True) for k, v in W.items()}
    B, NI, D = items.shape
    z = LW.logits(u, items, W, F64)[0]
    zo = z[(dom != 0).long(), torch.arange(B)]
    with torch.no_grad():
        top = torch.topk(zo[:, 1:], S + H, dim=1).indices[:, S:] + 1            # distinct random logits: no ties
        c = torch.cat((torch.zeros(B, 1, dtype=torch.long), top.sort(1).values), 1)
    zc = zo.gather(1, c)
    if kind == LW.SOFTMAX:
        L = (torch.logsumexp(zc, 1) - zc[:, 0]).mean()
    else:
        L = torch.nn.functional.softplus(zc[:, 1:] - zc[:, :1]).mean(1).mean()
    L.backward()
    return L, c[:, 1:], u.grad, items.grad, W


@pytest.mark.parametrize("kind", [LW.SOFTMAX, LW.BPR])
@pytest.mark.parametrize("B,NI,D,hid,H,S", CASES)
def test_against_autograd_over_topk_indices(B, NI, D, hid, H, S, kind):
    u, items, W, dom = _inputs(B, NI, D, hid)
    L, sel, du, ditems, Wg = _autograd(u, items, W, dom, kind, H, S)
    got = MR.launch(u, items, W, dom, kind, H, S, F64)
    assert torch.equal(got["sel"], sel)
    tol = dict(rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(got["loss_part"].sum(), L.detach(), **tol)
    torch.testing.assert_close(got["du"], du, **tol)
    torch.testing.assert_close(got["ditems"], ditems, **tol)
    torch.testing.assert_close(got["sc_dW1"].sum(0).reshape(hid, 2 * D), Wg["w1"].grad, **tol)
    torch.testing.assert_close(got["sc_db1"].sum(0), Wg["b1"].grad, **tol)
    torch.testing.assert_close(got["sc_dW2"].sum(0), Wg["w2"].grad, **tol)
    torch.testing.assert_close(got["sc_db2"].sum(0), Wg["b2"].grad, **tol)
    # the given-selection mode: the same outputs
    again = MR.launch(u, items, W, dom, kind, H, S, F64, sel=sel)
    assert all(torch.equal(again[k], got[k]) for k in got)


def test_ties_go_to_the_lower_position():
    zo = torch.zeros(2, 9, dtype=F64)
    for H, S in ((1, 0), (3, 0), (3, 2), (8, 0), (2, 6)):
        assert torch.equal(MR.select(zo, H, S), torch.arange(S + 1, S + H + 1).expand(2, H)), (H, S)
    # a tie between two positions below a larger logit
    zo = torch.tensor([[0.0, 1.0, 3.0, 1.0, 0.5, 1.0]], dtype=F64)
    assert MR.ranks(zo).tolist() == [[1, 0, 2, 4, 3]]
    assert MR.select(zo, 2, 1).tolist() == [[1, 3]]
    assert MR.select(zo, 2, 2).tolist() == [[3, 5]]


def test_through_the_launch_equal_logits_keep_the_first_positions():
    u, items, W, dom = _inputs(2, 9, 32, 8)
    W = dict(W, w2=torch.zeros(8, dtype=F64))
    got = MR.launch(u, items, W, dom, LW.SOFTMAX, 3, 2, F64)
    assert got["sel"].tolist() == [[3, 4, 5]] * 2
    torch.testing.assert_close(got["loss_part"].sum(), torch.log(torch.tensor(4.0, dtype=F64)))


@pytest.mark.parametrize("kind", [LW.SOFTMAX, LW.BPR])
def test_all_kept_is_the_listwise_reference_exactly(kind):
    for dtype in (F64, torch.float32):
        u, items, W, dom = _inputs(3, 9, 32, 8)
        full = LW.launch(u, items, W, dom, kind, dtype)
        got = MR.launch(u, items, W, dom, kind, 8, 0, dtype)
        assert got["sel"].tolist() == [list(range(1, 9))] * 3
        for k in full:
            assert torch.equal(got[k], full[k]), (k, dtype)


def test_skip_shifts_the_window():
    u, items, W, dom = _inputs(3, 12, 32, 8)
    zo = MR.own_rows(LW.logits(u, items, W, F64)[0], dom)
    order = torch.argsort(zo[:, 1:], 1, descending=True) + 1
    for H, S in ((3, 0), (3, 1), (3, 4), (2, 9)):
        assert torch.equal(MR.select(zo, H, S), order[:, S:S + H].sort(1).values), (H, S)
    a, b = MR.select(zo, 4, 0), MR.select(zo, 3, 1)
    for r in range(3):
        assert set(b[r].tolist()) < set(a[r].tolist())


@pytest.mark.parametrize("kind", [LW.SOFTMAX, LW.BPR])
def test_rows_not_kept_have_zero_gradient(kind):
    u, items, W, dom = _inputs(3, 12, 32, 8)
    got = MR.launch(u, items, W, dom, kind, 3, 1, F64)
    keep = MR.kept_mask(got["sel"], 12)
    own = (dom != 0).long()
    dz_own = got["dz"][own, torch.arange(3)]
    assert torch.equal(dz_own[~keep], torch.zeros(int((~keep).sum()), dtype=F64))
    assert torch.equal(got["dz"][1 - own, torch.arange(3)], torch.zeros(3, 12, dtype=F64))
    assert torch.equal(got["ditems"][~keep], torch.zeros(int((~keep).sum()), 32, dtype=F64))
    assert bool((dz_own[keep] != 0).all()) and bool((got["ditems"][keep].abs().sum(1) > 0).all())


def test_loss_on_p_is_the_launch_s_loss():
    u, items, W, dom = _inputs(3, 12, 32, 8)
    for kind in (LW.SOFTMAX, LW.BPR):
        got = MR.launch(u, items, W, dom, kind, 3, 1, F64)
        torch.testing.assert_close(MR.loss_on_p(got["p"][0], got["p"][1], dom, kind, got["sel"]), got["loss_part"].sum(), rtol=1e-9, atol=1e-12)


def test_select_refuses_a_window_past_the_negatives():
    with pytest.raises(ValueError):
        MR.select(torch.zeros(1, 5, dtype=F64), 3, 2)
    with pytest.raises(ValueError):
        MR.select(torch.zeros(1, 5, dtype=F64), 0, 0)
