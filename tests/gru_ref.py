"""Restatement of the reference's GRU4Rec (model_seq.py:56-113; isInC = isItC = isDR = False) for the tests: torch.nn.GRU + plain mean over
time + predictModule + the masked BCE of train_sr.py:203-212, with autograd, in any dtype (the tests use fp64).  Pinned to the reference by
tests/test_gru_ref_golden.py on tests/golden/g16_gru4rec.npz; every GPU test of the model compares against this file.

`gru_taps` is the same layer stepped by hand, returning what the kernels of csrc/gru.hip store (gi, h, the gates, ghn, hprev); it is
checked against nn.GRU here and carries the two mutants the kernel tests must be able to see."""
from collections import OrderedDict
from typing import Dict, Tuple

import torch

from oracle import amid_oracle as orc


def gru4rec_param_shapes(n_items: int, D: int, hid: int) -> "OrderedDict[str, Tuple[int, ...]]":
    """The reference's state_dict, in its order."""
    s: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    s["item_emb_layer.emb_item.weight"] = (n_items, D)
    for d in (1, 2):
        s[f"gru{d}.weight_ih_l0"] = (3 * D, D)
        s[f"gru{d}.weight_hh_l0"] = (3 * D, D)
        s[f"gru{d}.bias_ih_l0"] = (3 * D,)
        s[f"gru{d}.bias_hh_l0"] = (3 * D,)
    s["predictModule.fc.0.weight"] = (hid, 2 * D)
    s["predictModule.fc.0.bias"] = (hid,)
    s["predictModule.fc.2.weight"] = (1, hid)
    s["predictModule.fc.2.bias"] = (1,)
    return s


def gru_layer(x: torch.Tensor, w_ih: torch.Tensor, w_hh: torch.Tensor, b_ih: torch.Tensor, b_hh: torch.Tensor) -> torch.Tensor:
    """nn.GRU(D, D, 1, batch_first=True) from h0 = 0 on x [N, T, D] -> every step's output [N, T, D]; differentiable in all five."""
    D = x.shape[-1]
    m = torch.nn.GRU(D, D, 1, batch_first=True).to(x.dtype)
    h0 = torch.zeros(1, x.shape[0], D, dtype=x.dtype)
    out, _ = torch.func.functional_call(m, {"weight_ih_l0": w_ih, "weight_hh_l0": w_hh, "bias_ih_l0": b_ih, "bias_hh_l0": b_hh}, (x, h0))
    return out


def gru_taps(x: torch.Tensor, w_ih: torch.Tensor, w_hh: torch.Tensor, b_ih: torch.Tensor, b_hh: torch.Tensor, mutant: str = "") -> Dict[str, torch.Tensor]:
    """The layer stepped by hand.  gi [N, T, 3D]; h, ghn (= W_hn h_{t-1} + b_hn), hprev [N, T, D]; gates [N, T, 3D] = (r, z, n); gh_steps:
    the T tensors W_hh h_{t-1} + b_hh [N, 3D] (autograd leaves-in-the-middle for the gradient the kernels call dgh).
    mutant = "swap_rz": the r and z blocks of W_hh exchanged; "bhn_outside": b_hn added outside r * ( )."""
    N, T, D = x.shape
    if mutant == "swap_rz":
        w_hh = torch.cat((w_hh[D:2 * D], w_hh[:D], w_hh[2 * D:]), 0)
    gi = x @ w_ih.t() + b_ih
    h = torch.zeros(N, D, dtype=x.dtype)
    hs, gates, ghns, hprevs, ghs = [], [], [], [], []
    for t in range(T):
        gh = h @ w_hh.t() + b_hh
        ghs.append(gh)
        r = torch.sigmoid(gi[:, t, :D] + gh[:, :D])
        z = torch.sigmoid(gi[:, t, D:2 * D] + gh[:, D:2 * D])
        if mutant == "bhn_outside":
            n = torch.tanh(gi[:, t, 2 * D:] + r * (gh[:, 2 * D:] - b_hh[2 * D:]) + b_hh[2 * D:])
        else:
            n = torch.tanh(gi[:, t, 2 * D:] + r * gh[:, 2 * D:])
        hprevs.append(h)
        ghns.append(gh[:, 2 * D:])
        h = (1.0 - z) * n + z * h
        hs.append(h)
        gates.append(torch.cat((r, z, n), -1))
    st = lambda l: torch.stack(l, 1)      # noqa: E731
    return dict(gi=gi, h=st(hs), gates=st(gates), ghn=st(ghns), hprev=st(hprevs), gh_steps=ghs)


def gru4rec_forward(P, i_node, neg_samples, seq_d1, seq_d2):
    """GRU4Rec.forward: plain gathered rows (no positional table, no mask: the pad row is an ordinary row), one GRU per domain, the
    mean over all T outputs, predictModule on [positive | negatives].  Returns the two [B, 1 + neg] outputs."""
    table = P["item_emb_layer.emb_item.weight"]
    items = torch.cat((table[i_node].unsqueeze(1), table[neg_samples]), 1)
    u = []
    for d, seq in ((1, seq_d1), (2, seq_d2)):
        g = f"gru{d}."
        out = gru_layer(table[seq], P[g + "weight_ih_l0"], P[g + "weight_hh_l0"], P[g + "bias_ih_l0"], P[g + "bias_hh_l0"])
        u.append(out.mean(1))
    return orc.predict_module(u[0], u[1], items, P)


def loss_and_grads(P, batch, dtype=torch.float64):
    """(loss, (p1, p2), grads of every parameter; the table's dense) in `dtype`."""
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in P.items()}
    p1, p2 = gru4rec_forward(leaves, batch["i_node"], batch["neg_samples"], batch["seq_d1"], batch["seq_d2"])
    loss = orc.masked_bce_loss(p1, p2, batch["label"].to(dtype), batch["domain_id"])
    names = list(leaves)
    gs = torch.autograd.grad(loss, [leaves[n] for n in names], allow_unused=True)
    grads = {n: (g if g is not None else torch.zeros_like(leaves[n])) for n, g in zip(names, gs)}
    return loss.detach(), (p1.detach(), p2.detach()), grads


def golden_params(z) -> Dict[str, torch.Tensor]:
    """The fixture's parameters, regenerated from its seed (checksum-guarded)."""
    P = orc.random_params(gru4rec_param_shapes(int(z["n_items"]), int(z["D"]), int(z["hid"])), seed=int(z["param_seed"]))
    s = sum(float(v.double().sum()) for v in P.values())
    assert abs(s - float(z["param_sum"])) < 1e-9 * max(1.0, abs(s)), "random_params drifted from the fixture generator"
    return P
