"""tests/attention_ref.py in float64 against torch's own scaled_dot_product_attention and its autograd (an independent formulation: fused
softmax, the scale applied to the scores, -inf for masked keys), the dropout path against a hand-multiplied mask, and the two edges the
kernels treat specially: a row whose keys are ALL masked (uniform softmax, no score gradient) and T = 1."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import attention_ref as R

TOL = 1e-12


def _case(n, T, D, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, T, D, generator=g, dtype=torch.float64) for _ in range(4)]


def _sdpa(q, k, v, d_o, H, **kw):
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    qh, kh, vh = (R._heads(t, H) for t in leaves)
    o = F.scaled_dot_product_attention(qh, kh, vh, **kw).permute(0, 2, 1, 3).reshape(q.shape)
    o.backward(d_o)
    return dict(o=o.detach(), dq=leaves[0].grad, dk=leaves[1].grad, dv=leaves[2].grad)


def _close(got, want, names=("o", "dq", "dk", "dv")):
    for n in names:
        scale = float(want[n].abs().max())
        assert float((got[n] - want[n]).abs().max()) <= TOL * max(scale, 1.0), n


@pytest.mark.parametrize("T,D,H", [(1, 16, 1), (7, 32, 4), (17, 48, 3), (50, 64, 8), (64, 128, 8)])
def test_causal_equals_sdpa_and_its_autograd(T, D, H):
    q, k, v, d_o = _case(3, T, D, 10 + T)
    got = R.causal(q, k, v, H, d_o=d_o)
    _close(got, _sdpa(q, k, v, d_o, H, is_causal=True))
    # the statistics: row max of the scaled, masked scores and 1 / sum of exp(score - max), [n, T, H, 2]
    S = (R._heads(q, H) * math.sqrt(1.0 / (D // H))) @ R._heads(k, H).transpose(-1, -2)
    S = S.masked_fill(torch.triu(torch.ones(T, T, dtype=torch.bool), 1), float("-inf"))
    assert got["stats"].shape == (3, T, H, 2)
    assert torch.equal(got["stats"][..., 0], S.max(-1).values.permute(0, 2, 1))
    lse = torch.logsumexp(S, -1).permute(0, 2, 1)
    assert float((got["stats"][..., 0] - torch.log(got["stats"][..., 1]) - lse).abs().max()) <= TOL * float(lse.abs().max())


@pytest.mark.parametrize("T,D,H", [(1, 32, 1), (7, 64, 2), (17, 96, 3), (50, 128, 4), (64, 256, 8)])
def test_bidirectional_equals_sdpa_with_a_boolean_mask(T, D, H):
    q, k, v, d_o = _case(4, T, D, 20 + T)
    g = torch.Generator().manual_seed(T)
    keep = torch.rand(4, T, generator=g) > 0.3
    keep[:, 0] = True                                    # (a fully masked row is NaN in scaled_dot_product_attention: its own test below)
    keep[1] = True
    got = R.bidirectional(q, k, v, keep, H, d_o=d_o)
    _close(got, _sdpa(q, k, v, d_o, H, attn_mask=keep[:, None, None, :].expand(4, 1, T, T)))
    _close(R.bidirectional(q[1:2], k[1:2], v[1:2], None, H, d_o=d_o[1:2]), {n: t[1:2] for n, t in got.items()})      # no mask = all kept


def test_row_with_every_key_masked_is_uniform_and_has_no_score_gradient():
    T, D, H = 9, 64, 2
    q, k, v, d_o = _case(2, T, D, 3)
    keep = torch.ones(2, T, dtype=torch.bool)
    keep[0] = False
    got = R.bidirectional(q, k, v, keep, H, d_o=d_o)
    assert float((got["o"][0] - v[0].mean(0, keepdim=True)).abs().max()) <= TOL
    assert float(got["dq"][0].abs().max()) == 0.0 and float(got["dk"][0].abs().max()) == 0.0
    assert float((got["dv"][0] - d_o[0].sum(0, keepdim=True) / T).abs().max()) <= TOL * T
    assert torch.equal(got["stats"][0, ..., 0], torch.full((T, H), -1e9, dtype=torch.float64))
    assert torch.equal(got["stats"][0, ..., 1], torch.full((T, H), 1.0 / T, dtype=torch.float64))
    _close({n: t[1:] for n, t in got.items()}, _sdpa(q[1:], k[1:], v[1:], d_o[1:], H))


@pytest.mark.parametrize("form", ["causal", "bidirectional"])
def test_single_token(form):
    q, k, v, d_o = _case(2, 1, 32, 4)
    got = R.causal(q, k, v, 2, d_o=d_o) if form == "causal" else R.bidirectional(q, k, v, torch.ones(2, 1, dtype=torch.bool), 1, d_o=d_o)
    assert torch.equal(got["o"], v) and torch.equal(got["dv"], d_o)
    assert float(got["dq"].abs().max()) == 0.0 and float(got["dk"].abs().max()) == 0.0
    assert torch.equal(got["stats"][..., 1], torch.ones_like(got["stats"][..., 1]))


@pytest.mark.parametrize("form,p", [("causal", 0.5), ("bidirectional", 0.1)])
def test_dropout_is_the_hand_multiplied_mask(form, p):
    n, T, D, H = 3, 11, 32, 2
    hd = D // H
    q, k, v, d_o = _case(n, T, D, 5)
    g = torch.Generator().manual_seed(6)
    keep = torch.rand(n, H, T, T, generator=g) >= p
    key_keep = torch.rand(n, T, generator=g) > 0.3
    key_keep[:, 0] = True
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    qh, kh, vh = (R._heads(t, H) for t in leaves)
    if form == "causal":
        got = R.causal(q, k, v, H, keep=keep, p=p, d_o=d_o)
        bias = torch.zeros(T, T, dtype=torch.float64).masked_fill(torch.triu(torch.ones(T, T, dtype=torch.bool), 1), float("-inf"))
    else:
        got = R.bidirectional(q, k, v, key_keep, H, keep=keep, p=p, d_o=d_o)
        bias = torch.zeros(n, 1, 1, T, dtype=torch.float64).masked_fill(~key_keep[:, None, None, :], float("-inf"))
    A = torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(hd) + bias, -1)
    o = ((A * keep.double() / (1.0 - p)) @ vh).permute(0, 2, 1, 3).reshape(n, T, D)
    o.backward(d_o)
    _close(got, dict(o=o.detach(), dq=leaves[0].grad, dk=leaves[1].grad, dv=leaves[2].grad))
    no_drop = R.causal(q, k, v, H) if form == "causal" else R.bidirectional(q, k, v, key_keep, H)
    assert torch.equal(no_drop["stats"], got["stats"])          # the statistics are those of the softmax before dropout


def test_keep_masks_index_the_batch_row():
    """[b, h, i, j] with the row padded to whole Philox calls: sequence (g, b)'s mask does not depend on the batch size around it."""
    a = R.keep_masks_both(5, 2, 20, 7, 3, 1, 0.5)
    b = R.keep_masks_both(3, 2, 20, 7, 3, 1, 0.5)
    assert a.shape == (10, 2, 20, 20) and a.dtype == torch.bool
    assert torch.equal(a[:3], b[:3]) and torch.equal(a[5:8], b[3:])
    assert not torch.equal(a[:5], a[5:])
    assert 0.4 < float(a.float().mean()) < 0.6 and 0.85 < float(R.keep_masks(4, 4, 50, 7, 3, 0, 0, 0.1).float().mean()) < 0.95


@pytest.mark.parametrize("exp2", [False, True])
def test_float32_restatements_stay_near_float64(exp2):
    q, k, v, d_o = _case(3, 33, 64, 8)
    keep = torch.rand(3, 4, 33, 33, generator=torch.Generator().manual_seed(1)) >= 0.5
    r64 = R.causal(q.float(), k.float(), v.float(), 4, keep=keep, d_o=d_o.float())
    r32 = R.causal(q.float(), k.float(), v.float(), 4, torch.float32, keep=keep, d_o=d_o.float(), exp2=exp2)
    for n in ("o", "dq", "dk", "dv"):
        assert r32[n].dtype == torch.float32 and 0.0 < R.err(r32[n], r64[n]) < 2e-6, n
