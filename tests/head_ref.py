"""The head of a train step restated in plain torch, with the dtype a parameter: float64 is the reference of tests/test_gpu_head.py,
float32 on the CPU its yardstick.  The formulas are those of the header comments of include/amid_hip.h, amid_amd/csrc/head.hip and
head_fused.hip (reference: last_layernorm model_seq.py:385, the mean over T :432-434, predictModule.forward :40-54, the masked BCE of
train_sr.py:203-212, the doubly-robust objectives of train_sr_dr.py:216-221 and :392-394); every backward is written out, and
tests/test_head_ref.py holds the float64 form of all of it to torch.autograd through an independent formulation.

Shapes: x [2, B, T, D] (domain, batch row, time, feature), u [2, B, D], items [B, NI, D], labels [B, NI], domain_id [B],
W = dict(w1 [hid, 2D] (user half | item half), b1 [hid], w2 [hid], b2 [1]); p, dp and their kin [2, B, NI] (head of domain 1, of domain 2)."""
import torch

EPS = 1e-8                       # SASREC_LN_EPS


# ---------------------------------------------------------------------------- last LayerNorm + mean over time
def _normalise(x, eps):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)                 # biased
    rstd = 1.0 / torch.sqrt(var + eps)                           # eps inside the sqrt
    return (x - mu) * rstd, rstd


def lnmean(x, ln, dtype, eps=EPS):
    """u[g, b] = mean_t (xhat[g, b, t] * w_g + b_g); ln = (w [2, D], b [2, D]) or None: the plain mean."""
    x = x.to(dtype)
    if ln is None:
        return x.mean(2)
    xh, _ = _normalise(x, eps)
    w, b = ln[0].to(dtype), ln[1].to(dtype)
    return (xh * w[:, None, None, :] + b[:, None, None, :]).mean(2)


def lnmean_bwd(x, du, ln, dtype, eps=EPS):
    """dx [2, B, T, D], and part [2B, 2, D]: per sequence g * B + b, slot 0 = its share of d gamma (sum_t dy xhat), slot 1 of d beta (sum_t dy),
    with dy = du / T the gradient of every row of the sequence.  ln None: dx = du / T on every row, no part."""
    x, du = x.to(dtype), du.to(dtype)
    G, B, T, D = x.shape
    dy = (du / T)[:, :, None, :].expand(G, B, T, D)
    if ln is None:
        return dict(dx=dy.clone())
    xh, rstd = _normalise(x, eps)
    gy = dy * ln[0].to(dtype)[:, None, None, :]
    c1 = gy.mean(-1, keepdim=True)
    c2 = (gy * xh).mean(-1, keepdim=True)
    dx = rstd * (gy - c1 - xh * c2)
    part = torch.stack(((dy * xh).sum(2), dy.sum(2)), dim=2)     # [2, B, 2, D]
    return dict(dx=dx, ln_part=part.reshape(G * B, 2, D))


def layernorm_rows(x, w, b, dtype, eps=EPS):
    xh, _ = _normalise(x.to(dtype), eps)
    return xh * w.to(dtype) + b.to(dtype)


# ---------------------------------------------------------------------------- scorer
def scorer(u, items, W, dtype):
    """p_d[b, n] = sigmoid(w2 . relu(W1 [u_d[b] | item[b, n]] + b1) + b2); also the hidden pre-activations [2, B, NI, hid]."""
    u, items = u.to(dtype), items.to(dtype)
    w1, b1, w2, b2 = (W[k].to(dtype) for k in ("w1", "b1", "w2", "b2"))
    D = u.shape[-1]
    au = u @ w1[:, :D].t() + b1                                  # [2, B, hid]
    ci = items @ w1[:, D:].t()                                   # [B, NI, hid]
    pre = au[:, :, None, :] + ci[None]
    z = torch.relu(pre) @ w2 + b2
    return 1.0 / (1.0 + torch.exp(-z)), pre


def own_mask(domain_id, dtype):
    """[2, B]: 1 where head d is the one of the row's own domain."""
    own = (domain_id != 0).long()
    return torch.stack((own == 0, own == 1)).to(dtype)


def bce(p, y):
    """-(y log p + (1 - y) log(1 - p)) with the logs clamped at -100, and its derivative with the denominator clamped at 1e-12."""
    lp, l1p = torch.log(p).clamp_min(-100.0), torch.log(1.0 - p).clamp_min(-100.0)
    return -(y * lp + (1.0 - y) * l1p), (p - y) / ((1.0 - p) * p).clamp_min(1e-12)


def masked_bce(p, labels, domain_id, dtype):
    """The mean over B * NI of the BCE of the row's own head: loss_part [B] (its sum is the loss) and dLoss/dp [2, B, NI]."""
    p, y = p.to(dtype), labels.to(dtype)
    _, B, NI = p.shape
    m = own_mask(domain_id, dtype)[:, :, None]
    inv = torch.tensor(1.0 / (B * NI), dtype=dtype)
    val, _ = bce(p, y)
    dp = m * inv * (p - y) / ((1.0 - p) * p).clamp_min(1e-12)   # (in this order: torch's own backward multiplies first, then divides)
    return dict(loss_part=(val * m * inv).sum((0, 2)), dp=dp, bce=val)


def scorer_bwd(u, items, W, p, dp, dtype):
    """Per sample: da [B, 2, hid] (gradient of the user halves' pre-activations summed over the items), dc [B, NI, hid] (of the item halves',
    summed over the two heads), dw2 [B, hid], db2 [B]; du [2, B, D], ditems [B, NI, D]."""
    u, items, p, dp = u.to(dtype), items.to(dtype), p.to(dtype), dp.to(dtype)
    w1, w2 = W["w1"].to(dtype), W["w2"].to(dtype)
    D = u.shape[-1]
    _, pre = scorer(u, items, W, dtype)
    dz = dp * p * (1.0 - p)                                      # [2, B, NI]
    h = torch.relu(pre)
    g = (pre > 0).to(dtype) * dz[..., None] * w2                 # [2, B, NI, hid]
    da = g.sum(2).permute(1, 0, 2).contiguous()                  # [B, 2, hid]
    dc = g.sum(0)
    return dict(da=da, dc=dc, dw2=(dz[..., None] * h).sum((0, 2)), db2=dz.sum((0, 2)),
                du=g.sum(2) @ w1[:, :D], ditems=dc @ w1[:, D:])


def part_floats(D, hid):
    return (hid * 2 * D + 2 * hid + 1 + 3) & ~3                  # amid_scorer_part_floats


def vec_floats(NI, hid):
    return ((3 + NI) * hid + 1 + 3) & ~3                         # amid_scorer_vec_floats


def sc_part_rows(u, items, bw):
    """[B, hid * 2D + 2 hid + 1]: a sample's dW1 (hid x 2D) | db1 | dW2 | db2 (the row without its padding)."""
    u, items = u.to(bw["da"].dtype), items.to(bw["da"].dtype)
    B = items.shape[0]
    dw1u = torch.einsum("bdj,dbe->bje", bw["da"], u)
    dw1i = torch.einsum("bnj,bne->bje", bw["dc"], items)
    dw1 = torch.cat((dw1u, dw1i), dim=2)
    return torch.cat((dw1.reshape(B, -1), bw["da"].sum(1), bw["dw2"], bw["db2"][:, None]), dim=1)


def hidg_rows(bw):
    """[B, (3 + NI) hid + 1]: da [2][hid] | dc [NI][hid] | dW2 | db2 (the row without its padding)."""
    B = bw["dc"].shape[0]
    return torch.cat((bw["da"].reshape(B, -1), bw["dc"].reshape(B, -1), bw["dw2"], bw["db2"][:, None]), dim=1)


# ---------------------------------------------------------------------------- doubly-robust objectives
def move_ulps(t, n):
    """t moved by n units in the last place (n = 0, +1 or -1), towards +inf for n > 0."""
    return t if n == 0 else torch.nextafter(t, torch.full_like(t, float("inf") if n > 0 else float("-inf")))


def dr_loss(p, ips, g, labels, domain_id, ob_label, mode, w, dtype, c_ulps=0):
    """On the own head's p, ips, g of every row, c = BCE(p, y) (c_ulps: c moved by so many ulps first -- what another logf does to the result,
    tests/test_head_ref.py):
         mode 0: L = mean(c + w (c - g)^2 / ips)        mode 1: L = mean(g^2 + ob ((c^2 - g^2)^2) / ips)
    dp, dips, dg [2, B, NI] (zero on the other head) and loss_part [B, 3] = the rows' sums of c, (c - g)^2 / ips, g^2 + ob (c^2 - g^2)^2 / ips,
    each divided by B * NI."""
    p, ips, g, y = p.to(dtype), ips.to(dtype), g.to(dtype), labels.to(dtype)
    _, B, NI = p.shape
    m = own_mask(domain_id, dtype)[:, :, None]
    ob = torch.zeros(B, dtype=dtype) if ob_label is None else ob_label.to(dtype)
    ob = ob[None, :, None]
    inv = torch.tensor(1.0 / (B * NI), dtype=dtype)
    c, dc = bce(p, y)
    c = move_ulps(c, c_ulps)
    q = c * c - g * g
    if mode == 0:
        dp = (1.0 + 2.0 * w * (c - g) / ips) * dc
        dg = -2.0 * w * (c - g) / ips
        dips = -w * (c - g) * (c - g) / (ips * ips)
    else:
        dp = ob * 4.0 * q * c / ips * dc
        dg = 2.0 * g - ob * 4.0 * q * g / ips
        dips = -ob * q * q / (ips * ips)
    terms = torch.stack((c, (c - g) * (c - g) / ips, g * g + ob * q * q / ips), dim=-1)      # [2, B, NI, 3]
    return dict(dp=dp * inv * m, dips=dips * inv * m, dg=dg * inv * m, loss_part=(terms * m[..., None]).sum((0, 2)) * inv)
