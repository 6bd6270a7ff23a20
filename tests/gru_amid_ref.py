"""Restatement of the reference's GRU4Rec.forward with its three switches (model_seq.py:83-113: isInC :89-91, isItC :97-101, isDR :106-110)
for the tests, composed from pieces that are pinned already: tests/gru_ref.gru_layer (nn.GRU) and the oracle's inner_comp, inter_comp,
predict_module, masked_bce_loss and dr_losses.  Any dtype (the tests use fp64), with autograd.  Pinned to the reference by
tests/test_gru_amid_ref_golden.py on tests/golden/g17 .. g19; every GPU test of the variants compares against this file.

The taps are what the kernel tests need: per InterComp module s, softmax, gate (the oracle's), and u_raw (the plain means of the GRU
outputs), u (the mixed user vectors), Z (InnerComp's token group)."""
import glob
import os
from collections import OrderedDict
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from oracle import amid_oracle as orc
from tests.gru_ref import gru_layer


def gru4rec_amid_param_shapes(n_items: int, D: int, hid: int, bs: int, isInC: bool = False, isItC: bool = False,
                              isDR: bool = False) -> "OrderedDict[str, Tuple[int, ...]]":
    """The reference's state_dict, in its order (the constructor's, model_seq.py:62-78)."""
    s: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    s["item_emb_layer.emb_item.weight"] = (n_items, D)
    for comp, on in (("inc", isInC), ("itc", isItC)):
        for d in (1, 2) if on else ():
            s[f"{comp}_d{d}.trans_nn.weight"] = (D, D)
            s[f"{comp}_d{d}.trans_nn.bias"] = (D,)
            s[f"{comp}_d{d}.trans_bs.weight"] = (1, bs)
            s[f"{comp}_d{d}.trans_bs.bias"] = (1,)
    for d in (1, 2):
        s[f"gru{d}.weight_ih_l0"] = (3 * D, D)
        s[f"gru{d}.weight_hh_l0"] = (3 * D, D)
        s[f"gru{d}.bias_ih_l0"] = (3 * D,)
        s[f"gru{d}.bias_hh_l0"] = (3 * D,)
    for head in ("predictModule",) + (("predict_ips", "predict_gfunc") if isDR else ()):
        s[f"{head}.fc.0.weight"] = (hid, 2 * D)
        s[f"{head}.fc.0.bias"] = (hid,)
        s[f"{head}.fc.2.weight"] = (1, hid)
        s[f"{head}.fc.2.bias"] = (1,)
    return s


def gru4rec_amid_forward(P, i_node, neg_samples, seq_d1, seq_d2, isInC: bool = False, isItC: bool = False, isDR: bool = False,
                         threshold1: float = 0.5, threshold2: float = 0.5, taps: Optional[dict] = None):
    """GRU4Rec.forward: two outputs [B, 1 + neg], six with isDR."""
    table = P["item_emb_layer.emb_item.weight"]
    items = torch.cat((table[i_node].unsqueeze(1), table[neg_samples]), 1)                 # :85-86, :105
    e = [table[seq_d1], table[seq_d2]]                                                     # :87-88 plain rows: no positions, no mask
    if isInC:                                                                              # :89-91 the GRUs then step through 2T tokens
        e = [orc.inner_comp(e[g], P, f"inc_d{g + 1}", threshold1, taps) for g in (0, 1)]
        if taps is not None:
            taps["Z"] = torch.stack([e[g][0, e[g].shape[1] // 2:].detach() for g in (0, 1)])
    h = [gru_layer(e[g], *(P[f"gru{g + 1}.{n}_l0"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))) for g in (0, 1)]      # :92-95
    f = h
    if isItC:                                                                              # :97-101 both from the un-mixed outputs
        f = [orc.inter_comp(h[0], h[1], P, "itc_d1", threshold2, taps), orc.inter_comp(h[1], h[0], P, "itc_d2", threshold2, taps)]
    u = [f[0].mean(1), f[1].mean(1)]                                                       # :102-104 over ALL steps (2T with either module)
    if taps is not None:
        taps.update(h=torch.stack([x.detach() for x in h]), u_raw=torch.stack([x.mean(1).detach() for x in h]),
                    u=torch.stack([x.detach() for x in u]))
        if isItC:
            taps.update(s=taps["itc_d1"]["s"], softmax=taps["itc_d1"]["softmax"], gate=taps["itc_d1"]["gate"])
    outs = orc.predict_module(u[0], u[1], items, P)
    if isDR:                                                                               # :106-110
        outs = outs + orc.predict_module(u[0], u[1], items, P, "predict_ips") + orc.predict_module(u[0], u[1], items, P, "predict_gfunc")
    return outs


def loss_and_grads(P, batch, dtype=torch.float64, which: str = "", dr_e_w: float = 0.1, taps: Optional[dict] = None, **flags):
    """(loss, outputs, grads of every parameter; the table's dense) in `dtype`.  which = "": the masked BCE of train_sr.py:203-212 on the
    first two outputs; "e": loss_cls + dr_e_w * loss_dr_e (train_sr_dr.py:216-221); "r": loss_dr_r with ob_label (:392-394)."""
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in P.items()}
    outs = gru4rec_amid_forward(leaves, batch["i_node"], batch["neg_samples"], batch["seq_d1"], batch["seq_d2"], taps=taps, **flags)
    if which:
        _, _, tot, lr_ = orc.dr_losses(outs, batch["label"].to(dtype), batch["domain_id"], batch.get("ob_label"), dr_e_w)
        loss = tot if which == "e" else lr_
    else:
        loss = orc.masked_bce_loss(outs[0], outs[1], batch["label"].to(dtype), batch["domain_id"])
    names = list(leaves)
    gs = torch.autograd.grad(loss, [leaves[n] for n in names], allow_unused=True)
    grads = {n: (g if g is not None else torch.zeros_like(leaves[n])) for n, g in zip(names, gs)}
    return loss.detach(), tuple(o.detach() for o in outs), grads


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name: str):
    """(z: every array of NAME.npz and its NAME.partK.npz files, the parameters, the batch) of a fixture of make_golden_gru_amid.py."""
    z = {}
    for path in [os.path.join(GOLDEN, name + ".npz")] + sorted(glob.glob(os.path.join(GOLDEN, name + ".part*.npz"))):
        with np.load(path, allow_pickle=False) as f:
            z.update({k: f[k] for k in f.files})
    batch = {k[2:]: torch.from_numpy(z[k]) for k in z if k.startswith("B/")}
    batch["label"] = torch.from_numpy(z["labels"])
    if "ob_label" in z:
        batch["ob_label"] = torch.from_numpy(z["ob_label"])
    return z, golden_params(z), batch


def golden_flags(z) -> Dict[str, object]:
    return dict(isInC=bool(z["isInC"]), isItC=bool(z["isItC"]), isDR=bool(z["isDR"]), threshold1=float(z["threshold1"]),
                threshold2=float(z["threshold2"]))


def golden_params(z) -> Dict[str, torch.Tensor]:
    """The fixture's parameters: regenerated from its seed (checksum-guarded), then the generator's scaling of the tensors it names."""
    fl = golden_flags(z)
    shapes = gru4rec_amid_param_shapes(int(z["n_items"]), int(z["D"]), int(z["hid"]), int(z["bs"]), fl["isInC"], fl["isItC"], fl["isDR"])
    P = orc.random_params(shapes, seed=int(z["param_seed"]))
    scale_params(P, float(z["table_scale"]), float(z["gru_scale"]))
    s = sum(float(v.double().sum()) for v in P.values())
    assert abs(s - float(z["param_sum"])) < 1e-9 * max(1.0, abs(s)), "random_params drifted from the fixture generator"
    return P


def scale_params(P, table_scale: float, gru_scale: float) -> None:
    """What the golden generator does to random_params' draw so that the gates split: the table and the GRU weights scaled in place."""
    P["item_emb_layer.emb_item.weight"].mul_(table_scale)
    for k in P:
        if k.startswith("gru") and "weight" in k:
            P[k].mul_(gru_scale)
