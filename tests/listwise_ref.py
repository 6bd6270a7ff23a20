"""The restatement of csrc/head_listwise.hip's launch (amid_scorer_listwise_fwd_bwd_f32) in plain torch on the CPU, in the dtype asked for:
float64 is the reference of tests/test_gpu_listwise.py (held to torch.autograd by tests/test_listwise_ref.py), float32 runs the same
formulas and gives the error a float32 evaluation may have (the e_f32 of the bar).

    z_d[b, n] = w2 . relu(W1 [u_d[b] | item[b, n]] + b1) + b2,   p = sigmoid(z);   the objective reads the own domain's z only
    kind 1 (softmax):  L_b = lse_n z[n] - z[0],                       dz[n] = exp(z[n] - lse) - [n == 0]
    kind 2 (BPR):      L_b = (1 / K) sum_{n >= 1} softplus(z[n] - z[0]),  dz[n] = sigmoid(z[n] - z[0]) / K,  dz[0] = -sum_{n >= 1} dz[n]
    loss_part[b] = L_b / B,  dz scaled by 1 / B;  the scorer's backward from dz (no p (1 - p) anywhere).
"""
import functools

import torch

from tests import head_ref as R

F64, F32 = torch.float64, torch.float32
SOFTMAX, BPR = 1, 2
KINDS = {"softmax": SOFTMAX, "bpr": BPR}


def logits(u, items, W, dtype):
    """z [2, B, NI] and the hidden pre-activations [2, B, NI, hid] (R.scorer without the sigmoid)."""
    u, items = u.to(dtype), items.to(dtype)
    w1, b1, w2, b2 = (W[k].to(dtype) for k in ("w1", "b1", "w2", "b2"))
    D = u.shape[-1]
    pre = (u @ w1[:, :D].t() + b1)[:, :, None, :] + (items @ w1[:, D:].t())[None]
    return torch.relu(pre) @ w2 + b2, pre


def objective(z, domain_id, kind, dtype):
    """z [2, B, NI] -> loss_part [B] (its sum is the loss) and dLoss/dz [2, B, NI] (the other domain's rows 0)."""
    z = z.to(dtype)
    _, B, NI = z.shape
    own = (domain_id != 0).long()
    zo = z[own, torch.arange(B)]                                 # [B, NI] the own domain's logits
    if kind == SOFTMAX:
        m = zo.max(1, keepdim=True).values
        lse = m + torch.log(torch.exp(zo - m).sum(1, keepdim=True))
        L = (lse - zo[:, :1])[:, 0]
        dzo = torch.exp(zo - lse)
        dzo[:, 0] = dzo[:, 0] - 1.0
    elif kind == BPR:
        K = NI - 1
        x = zo[:, 1:] - zo[:, :1]
        L = (x.clamp_min(0.0) + torch.log1p(torch.exp(-x.abs()))).sum(1) / K
        g = (1.0 / (1.0 + torch.exp(-x))) / K
        dzo = torch.cat((-g.sum(1, keepdim=True), g), dim=1)
    else:
        raise ValueError(kind)
    dz = torch.zeros_like(z)
    dz[own, torch.arange(B)] = dzo / B
    return dict(loss_part=L / B, dz=dz)


def objective_on_p(p, domain_id, kind, dtype):
    """The same on the scorer's outputs p = sigmoid(z) (the engine tests' oracles return p): z = logit(p)."""
    p = p.to(dtype)
    return objective(torch.log(p) - torch.log1p(-p), domain_id, kind, dtype)


def loss_on_p(p1, p2, domain_id, kind):
    """The batch's objective as a differentiable torch expression of the two outputs p = sigmoid(z) [B, NI] a model's forward returns
    (z = logit(p)): the mean over the rows of L_b on the own domain's logits.  For the engine tests' float64 oracles (autograd)."""
    B = p1.shape[0]
    p = torch.stack((p1, p2))[(domain_id != 0).long(), torch.arange(B)]
    z = torch.log(p) - torch.log1p(-p)
    if kind == SOFTMAX:
        return (torch.logsumexp(z, 1) - z[:, 0]).mean()
    if kind == BPR:
        return torch.nn.functional.softplus(z[:, 1:] - z[:, :1]).mean(1).mean()
    raise ValueError(kind)


def scorer_bwd_dz(u, items, W, pre, dz, dtype):
    """R.scorer_bwd from the gradient on the logits."""
    w1, w2 = W["w1"].to(dtype), W["w2"].to(dtype)
    D = u.shape[-1]
    pre, dz = pre.to(dtype), dz.to(dtype)
    h = torch.relu(pre)
    g = (pre > 0).to(dtype) * dz[..., None] * w2                 # [2, B, NI, hid]
    da = g.sum(2).permute(1, 0, 2).contiguous()
    dc = g.sum(0)
    return dict(da=da, dc=dc, dw2=(dz[..., None] * h).sum((0, 2)), db2=dz.sum((0, 2)), du=g.sum(2) @ w1[:, :D], ditems=dc @ w1[:, D:])


def launch(u, items, W, domain_id, kind, dtype):
    """Every output of the launch by name: z, p, loss_part, dz, du, ditems and the per-row partials sc_dW1, sc_db1, sc_dW2, sc_db2."""
    z, pre = logits(u, items, W, dtype)
    ob = objective(z, domain_id, kind, dtype)
    bw = scorer_bwd_dz(u, items, W, pre, ob["dz"], dtype)
    D, hid = u.shape[-1], W["b1"].numel()
    rows = R.sc_part_rows(u.to(dtype), items, bw)
    o = hid * 2 * D
    return dict(z=z, p=1.0 / (1.0 + torch.exp(-z)), loss_part=ob["loss_part"], dz=ob["dz"], du=bw["du"], ditems=bw["ditems"],
                sc_dW1=rows[:, :o], sc_db1=rows[:, o:o + hid], sc_dW2=rows[:, o + hid:o + 2 * hid], sc_db2=rows[:, o + 2 * hid:])


# ---------------------------------------------------------------------------- cases (the input conditions of tests/test_gpu_head.py)
MAX_SEED_STEPS = 8
MAX_NUDGES = 64


def _margin(u, items, W):
    """Hidden pre-activations in float64 and twice the float32 bound of their 2D-term dot products (test_gpu_head.relu_margin_ok's)."""
    from tests.test_gpu_head import operands
    v, w1 = operands(u, items), W["w1"].double()
    return v @ w1.t() + W["b1"].double(), 2 * (v.shape[-1] + 2) * 2.0 ** -24 * (v.abs() @ w1.abs().t())


def _nudge(u, items, W):
    """At a thousand candidates a few of the 2 B NI hid pre-activations fall inside the margin whatever the seed: move those items' rows along
    the unit's item weights, away from 0 by four bounds, until none does (the conditions are then CHECKED by the caller as for any case)."""
    items = items.clone()
    w1i = W["w1"][:, u.shape[-1]:].double()
    for _ in range(MAX_NUDGES):
        z, bound = _margin(u, items, W)
        bad = (z.abs() <= bound).nonzero()
        if bad.numel() == 0:
            break
        for d, b, n, j in bad.tolist():
            step = (1.0 if z[d, b, n, j] >= 0 else -1.0) * 4 * float(bound[d, b, n, j]) + 0.0
            items[b, n] = (items[b, n].double() + step * w1i[j] / (w1i[j] @ w1i[j])).float()
    return items


@functools.lru_cache(maxsize=None)
def case(B, NI, D, hid, dom="mixed", saturate=False):
    """Inputs of a launch -- u [2, B, D], items [B, NI, D], the scorer W, domain ids (all 0, all 1 or mixed) -- that meet head_ref's input
    conditions: every hidden pre-activation away from 0 by twice the fp32 dot bound, every p in (0.02, 0.98).  saturate: b2 = +40 afterwards
    (every p == 1.0f in float32).  Deterministic from the arguments."""
    from tests.test_gpu_head import draw_scorer, fit_b1, in_range, mixed_domain, relu_margin_ok
    for step in range(MAX_SEED_STEPS + 1):
        g = torch.Generator().manual_seed(100000 * B + 100 * NI + D + hid + 7919 * step + 17)
        rn = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
        u = 0.5 * rn(2, B, D) + 0.3 * rn(2, 1, D)
        items = 0.7 * rn(B, NI, D)
        W = draw_scorer(g, D, hid)
        W = fit_b1(u, items, dict(W, w2=W["w2"] * 0.85 ** step))       # (a thousand logits a row: the later steps narrow their spread)
        items = _nudge(u, items, W)
        if relu_margin_ok(u, items, W) and in_range(R.scorer(u, items, W, F64)[0]):
            break
    else:
        raise AssertionError(f"no seed within {MAX_SEED_STEPS} steps meets the ReLU margin and the value range")
    if saturate:
        W = dict(W, b2=torch.tensor([40.0]))
    return dict(u=u, items=items, W=W, domain_id=mixed_domain(B, dom), steps=step)


@functools.lru_cache(maxsize=None)
def refs(B, NI, D, hid, dom, kind, saturate=False):
    """(float64, float32) restatements of a case's launch; computed once, shared, not to be modified."""
    c = case(B, NI, D, hid, dom, saturate)
    return tuple(launch(c["u"], c["items"], c["W"], c["domain_id"], kind, t) for t in (F64, F32))
