"""The two attention cores restated in plain torch, with the dtype a parameter: float64 is the reference of
tests/test_gpu_attention_live.py and of the two attention tests of tests/test_gpu_kernels.py, float32 on the CPU its yardstick.

causal (SASRec, nn.MultiheadAttention as called at model_seq.py:374):   softmax((q sqrt(1/hd)) k^T + causal(-inf)) -> dropout -> . v
bidirectional (BERT4Rec, Attention.forward model_seq.py:149-162):       softmax(masked_fill(q k^T / sqrt(hd), ~key_keep, -1e9)) -> dropout -> . v

Shapes: q, k, v, d_o [n_seq, T, D]; key_keep bool [n_seq, T] (one row per SEQUENCE: the caller repeats a batch's [B, T] mask for both
domains); keep bool [n_seq, H, T, T] dropout keep decisions (None: no dropout), p the dropout rate.  Every function returns a dict with
o [n_seq, T, D], stats [n_seq, T, H, 2] = (row max of the scaled and masked scores, 1 / row sum of exp(score - max)) as the kernels
store them, and -- with d_o -- dq, dk, dv by autograd.

exp2 = True evaluates the exponential as exp2(x * log2(e)) with the product rounded to `dtype`: what the matrix-core kernels' one-instruction
exponential does by design (fast_exp, csrc/attention_mfma.h).  Its derivative is taken as the value itself, as for exp.
tests/test_attention_ref.py holds the float64 form to torch's scaled_dot_product_attention and its autograd."""
import math

import numpy as np
import torch

from oracle import amid_oracle as orc

LOG2E = 1.4426950408889634
FLOOR = 2.0 ** -22


class _Exp2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y = torch.exp2(x * torch.tensor(LOG2E, dtype=x.dtype))
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0]


def _heads(t, H):
    n, T, D = t.shape
    return t.reshape(n, T, H, D // H).permute(0, 2, 1, 3)


def _core(S, vh, keep, p, exp2):
    """softmax over the last axis of S [n, H, T, T] written out (max, exp, sum), dropout, . v; returns o [n, T, D] and stats [n, T, H, 2]"""
    m = S.detach().max(-1, keepdim=True).values
    e = _Exp2.apply(S - m) if exp2 else torch.exp(S - m)
    rl = 1.0 / e.sum(-1, keepdim=True)
    A = e * rl
    if keep is not None:
        A = A * keep.to(S.dtype) * (1.0 / (1.0 - p))
    n, H, T, hd = vh.shape
    o = (A @ vh).permute(0, 2, 1, 3).reshape(n, T, H * hd)
    stats = torch.cat((m, rl.detach()), -1).permute(0, 2, 1, 3).contiguous()      # [n, H, T, 2] -> [n, T, H, 2]
    return o, stats


def _run(form, q, k, v, d_o, dtype):
    leaves = [t.detach().to(dtype).clone().requires_grad_(d_o is not None) for t in (q, k, v)]
    o, stats = form(*leaves)
    out = dict(o=o.detach(), stats=stats)
    if d_o is not None:
        o.backward(d_o.to(dtype))
        out.update(dq=leaves[0].grad, dk=leaves[1].grad, dv=leaves[2].grad)
    return out


def causal(q, k, v, H, dtype=torch.float64, keep=None, p=0.5, d_o=None, exp2=False):
    T, hd = q.shape[1], q.shape[2] // H
    above = torch.triu(torch.ones(T, T, dtype=torch.bool), 1)

    def form(qq, kk, vv):
        S = (_heads(qq, H) * torch.tensor(math.sqrt(1.0 / hd), dtype=dtype)) @ _heads(kk, H).transpose(-1, -2)
        return _core(S.masked_fill(above, float("-inf")), _heads(vv, H), keep, p, exp2)
    return _run(form, q, k, v, d_o, dtype)


def bidirectional(q, k, v, key_keep, H, dtype=torch.float64, keep=None, p=0.1, d_o=None, exp2=False):
    hd = q.shape[2] // H

    def form(qq, kk, vv):
        S = (_heads(qq, H) @ _heads(kk, H).transpose(-1, -2)) / torch.tensor(math.sqrt(hd), dtype=dtype)
        if key_keep is not None:
            S = S.masked_fill(~key_keep[:, None, None, :], -1e9)
        return _core(S, _heads(vv, H), keep, p, exp2)
    return _run(form, q, k, v, d_o, dtype)


def keep_masks(B, H, T, seed, step, g, layer, p):
    """bool [B, H, T, T]: the keep decisions of domain g's encoder, indexed [b, h, i, j] with b the BATCH ROW and the row padded to whole
    Philox calls (oracle.attn_row_stride) -- the indexing of the kernels' counter RNG (csrc/rng.h)."""
    TP = orc.attn_row_stride(T, p)
    m = orc.philox_keep_flat(B * H * T * TP, seed, orc.site_id(g, layer, orc.SITE_ATTN), step, p)
    return torch.from_numpy(np.ascontiguousarray(m.reshape(B, H, T, TP)[..., :T])) != 0


def keep_masks_both(B, H, T, seed, step, layer, p):
    """bool [2 B, H, T, T] for the sequences g * B + b"""
    return torch.cat([keep_masks(B, H, T, seed, step, g, layer, p) for g in range(2)])


def err(x, r):
    """max|x - r| / max|r|"""
    x, r = x.double().cpu(), r.double().cpu()
    return float((x - r).abs().max() / r.abs().max())
