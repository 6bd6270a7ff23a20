"""The restatement of csrc/head_mined.hip's launch (amid_scorer_mined_fwd_bwd_f32) in plain torch on the CPU, built on
tests/listwise_ref.py: float64 is the reference of tests/test_gpu_mined.py (held to torch.autograd by tests/test_mined_ref.py), float32 runs
the same formulas and gives the error a float32 evaluation may have.

    z [2, B, NI] as listwise_ref.logits; zo = the own domain's row; the negatives are the positions 1 .. M = NI - 1
    rank(n) = #{ j in 1 .. M : zo[j] > zo[n] or (zo[j] == zo[n] and j < n) };  n is kept iff S <= rank(n) < S + H
    c = [0] + kept positions ascending (NC = 1 + H);  sel [B, H] = c[1:]
    the objective and the scorer's backward are listwise_ref's on the candidates items[b, c] (NI -> NC, BPR's 1 / K -> 1 / H);
    dz and ditems are scattered back to [.., NI, ..] with zeros at the positions that were not kept.
The selection is a constant: no gradient flows through it.  launch(..., sel=given) takes a selection instead of computing it (the GPU test
evaluates the reference on the kernel's own selection)."""
import functools

import torch

from tests import head_ref as R
from tests import listwise_ref as LW

F64, F32 = LW.F64, LW.F32
SOFTMAX, BPR = LW.SOFTMAX, LW.BPR


def ranks(zo):
    """zo [B, NI] -> rank [B, M] of the negatives 1 .. M by the rule (entry n - 1 is position n's)."""
    neg = zo[:, 1:]
    M = neg.shape[1]
    a, b = neg[:, None, :], neg[:, :, None]                      # a: z[j] along the last axis, b: z[n]
    j, n = torch.arange(M)[None, None, :], torch.arange(M)[None, :, None]
    return ((a > b) | ((a == b) & (j < n))).sum(2)


def select(zo, H, S):
    """sel [B, H] (int64): the kept positions in 1 .. M, ascending."""
    r = ranks(zo)
    B, M = r.shape
    if not (H >= 1 and S >= 0 and S + H <= M):
        raise ValueError((H, S, M))
    kept = (r >= S) & (r < S + H)
    assert bool((kept.sum(1) == H).all())
    return (kept.nonzero()[:, 1] + 1).reshape(B, H)


def own_rows(z, domain_id):
    return z[(domain_id != 0).long(), torch.arange(z.shape[1])]


def launch(u, items, W, domain_id, kind, H, S, dtype, sel=None):
    """Every output of the launch by name: z (both domains, [2, B, NI]), p, sel, loss_part, dz, du, ditems, sc_dW1, sc_db1, sc_dW2, sc_db2.
    sel given: that selection ([B, H], positions in 1 .. M ascending) instead of the rule on this dtype's logits."""
    B, NI, D = items.shape
    hid = W["b1"].numel()
    z, _ = LW.logits(u, items, W, dtype)
    if sel is None:
        sel = select(own_rows(z, domain_id), H, S)
    sel = sel.long()
    c = torch.cat((torch.zeros(B, 1, dtype=torch.long), sel), 1)                    # [B, NC]
    items_c = torch.gather(items, 1, c[:, :, None].expand(B, c.shape[1], D))
    zc, pre_c = LW.logits(u, items_c, W, dtype)
    ob = LW.objective(zc, domain_id, kind, dtype)
    bw = LW.scorer_bwd_dz(u, items_c, W, pre_c, ob["dz"], dtype)
    rows = R.sc_part_rows(u.to(dtype), items_c, bw)
    dz = torch.zeros(2, B, NI, dtype=dtype).scatter_(2, c[None].expand(2, B, c.shape[1]), ob["dz"])
    ditems = torch.zeros(B, NI, D, dtype=dtype).scatter_(1, c[:, :, None].expand(B, c.shape[1], D), bw["ditems"])
    o = hid * 2 * D
    return dict(z=z, p=1.0 / (1.0 + torch.exp(-z)), sel=sel, loss_part=ob["loss_part"], dz=dz, du=bw["du"], ditems=ditems,
                sc_dW1=rows[:, :o], sc_db1=rows[:, o:o + hid], sc_dW2=rows[:, o + hid:o + 2 * hid], sc_db2=rows[:, o + 2 * hid:])


def kept_mask(sel, NI):
    """[B, NI] bool: column 0 and the kept positions."""
    m = torch.zeros(sel.shape[0], NI, dtype=torch.bool)
    m[:, 0] = True
    return m.scatter_(1, sel.long(), True)


def loss_on_p(p1, p2, domain_id, kind, sel):
    """The batch's mined objective as a differentiable torch expression of a model's two outputs p = sigmoid(z) [B, NI] under a GIVEN selection
    sel [B, H]: listwise_ref.loss_on_p on the columns [0] + sel.  For the engine tests' float64 oracles (autograd)."""
    B = p1.shape[0]
    c = torch.cat((torch.zeros(B, 1, dtype=torch.long), sel.long()), 1)
    return LW.loss_on_p(torch.gather(p1, 1, c), torch.gather(p2, 1, c), domain_id, kind)


@functools.lru_cache(maxsize=None)
def case_z64(B, NI, D, hid, dom, saturate=False):
    """The float64 logits [2, B, NI] of listwise_ref's case; computed once, shared, not to be modified."""
    c = LW.case(B, NI, D, hid, dom, saturate)
    return LW.logits(c["u"], c["items"], c["W"], F64)[0]
