"""The float64 restatement of csrc/diversify.hip's operation (greedy Maximal Marginal Relevance over one row's list) in plain torch on the
CPU, and the per-entry bound on what fp32 may differ from it.

The operation: an entry is absent if its id is outside [0, n_rows) or its relevance is NaN; the shortlist is the M best present entries
(larger rel first, ties to the lower id, then the lower position); pick 1 is its head (value = lam * rel, max_sim = 0); pick j >= 2 is,
among the shortlist entries not picked whose id differs from every picked id, the largest v = (lam * rel) - ((1 - lam) * m), m = the
largest sim(c, s) over the picked s (ties: lower id, then lower position; a NaN v is never picked); it stops at K picks or when nothing
remains.  sim is the dot product, or the cosine with 1 / max(|row|, 1e-8) for the inverse norms.  lam is the fp32 number the kernel gets and
1 - lam is formed in fp32, as the definition says; everything else is float64 on the fp32 inputs.

The bound (mmr_row(..., with_bound=True)), from the order of operations the kernel documents, with u = 2^-24 and the standard model
|fl(a o b) - a o b| <= u |a o b|, gamma_n = n u / (1 - n u):
  dot      one fmaf chain of D terms from 0:                   |dot^ - dot| <= gamma_D sum |a_i b_i|
  inv      ss = eight fmaf chains of D / 8 squares joined by three levels of additions, all terms >= 0, so ss^ = ss (1 + e),
           |e| <= gamma_(D/8+3); sqrt halves it; sqrtf and the division are taken as within 2 u each (correctly rounded they are
           within u):                                          |inv^ - inv| <= rho inv,  rho = gamma_(D/8+3) / 2 + 4 u
  cosine   (dot^ * inv_c^) * inv_s^, two roundings:            |cos^ - cos| <= (gamma_D sum |a_i b_i| + |dot| (2 rho + 2 u)) inv_c inv_s
  m        a maximum of perturbed numbers moves by at most the largest perturbation: E_m(c) = max over the picked s of the line above
  v        fl(fl(lam rel) - fl(oml m^)):                       E_v <= oml E_m (1 + 2 u) + 2 u (|lam rel| + |oml m|)
each times (1 + 1e-3) for the second-order terms left out."""
import torch

U = 2.0 ** -24
SLACK = 1.0 + 1e-3
F64 = torch.float64


def gamma(n):
    return n * U / (1.0 - n * U)


def lex_order(*keys):
    """Indices that sort by keys[0] ascending, ties by keys[1], ... (stable sorts from the least significant key)."""
    idx = torch.arange(keys[0].numel())
    for key in reversed(keys):
        idx = idx[torch.sort(key[idx], stable=True).indices]
    return idx


def shortlist(ids, rel, n_rows, M):
    """Positions of the M best present entries of a list, in shortlist order."""
    ids, rel = torch.as_tensor(ids, dtype=torch.int64), torch.as_tensor(rel, dtype=torch.float32)
    at = torch.nonzero((ids >= 0) & (ids < n_rows) & ~torch.isnan(rel)).reshape(-1)
    return at[lex_order(-rel[at].to(F64), ids[at], at)][:M]


def mmr_row(ids, rel, table, metric, lam, K, M, with_bound=False):
    """One row.  ids int64 [n], rel float32 [n], table float32 [n_rows, D], metric 0 (dot) / 1 (cosine).  Returns a dict of K-long lists:
    ids, rel, value, max_sim, positions (padding -1 / -inf / -inf / -inf / -1); with_bound adds e_value and e_max_sim (the bound at each
    pick) and `margins`: for every pick j >= 2, (v_best - v_c - E_v(best) - E_v(c)) minimised over the other candidates c, and
    (v_best - v_second) - 2 max(E_v(best), E_v(second)) -- fp32 picks the same entry when both are positive."""
    ids, rel = torch.as_tensor(ids, dtype=torch.int64), torch.as_tensor(rel, dtype=torch.float32)
    n_rows, D = table.shape
    NEG = float("-inf")
    out = {"ids": [-1] * K, "rel": [NEG] * K, "value": [NEG] * K, "max_sim": [NEG] * K, "positions": [-1] * K, "e_value": [0.0] * K,
           "e_max_sim": [0.0] * K, "margins": []}
    sl = shortlist(ids, rel, n_rows, M)
    m = sl.numel()
    if m == 0:
        return out
    sid, r = ids[sl], rel[sl].to(F64)
    X = table[sid].to(F64)
    lam64 = float(torch.tensor(lam, dtype=torch.float32))
    oml = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(lam, dtype=torch.float32))
    G = X @ X.T
    A = X.abs() @ X.abs().T if with_bound else None
    if metric == 1:
        inv = 1.0 / torch.clamp(torch.sqrt((X * X).sum(1)), min=1e-8)
        S = (G * inv[:, None]) * inv[None, :]                              # S[c, s]: query c, candidate s
        if with_bound:
            rho = gamma(D // 8 + 3) / 2 + 4 * U
            E = (gamma(D) * A + G.abs() * (2 * rho + 2 * U)) * inv[:, None] * inv[None, :] * SLACK
    else:
        S = G
        if with_bound:
            E = gamma(D) * A * SLACK
    alive = torch.ones(m, dtype=torch.bool)
    run = torch.full((m,), NEG, dtype=F64)
    e_m = torch.zeros(m, dtype=F64)
    lr = lam64 * r
    p, value, ms, ev_p, em_p = 0, float(lr[0]), 0.0, U * abs(float(lr[0])) * SLACK, 0.0
    for j in range(K):
        if j > 0:
            v = lr - oml * run
            cand = torch.nonzero(alive & ~torch.isnan(v)).reshape(-1)
            if cand.numel() == 0:
                break
            order = cand[lex_order(-v[cand], sid[cand], sl[cand])]
            p = int(order[0])
            value, ms = float(v[p]), float(run[p])
            if with_bound:
                e_v = (oml * e_m * (1 + 2 * U) + 2 * U * (lr.abs() + (oml * run).abs())) * SLACK
                ev_p, em_p = float(e_v[p]), float(e_m[p])
                if order.numel() > 1:
                    rest = order[1:]
                    second = int(order[1])
                    out["margins"].append((float((v[p] - v[rest] - e_v[p] - e_v[rest]).min()),
                                           float(v[p] - v[second] - 2 * max(e_v[p], e_v[second]))))
        out["ids"][j], out["rel"][j], out["value"][j], out["max_sim"][j], out["positions"][j] = int(sid[p]), float(r[p]), value, ms, int(sl[p])
        out["e_value"][j], out["e_max_sim"][j] = ev_p, em_p
        alive &= sid != sid[p]
        run = torch.maximum(run, S[:, p])
        if with_bound:
            e_m = torch.maximum(e_m, E[:, p])
    return out


def mmr_lists(items, offsets, rel, table, metric, lam, K, M, with_bound=False):
    """Every row of ragged lists (items [n], offsets [B + 1], rel [n]): a list of mmr_row results."""
    items, rel = torch.as_tensor(items, dtype=torch.int64), torch.as_tensor(rel, dtype=torch.float32)
    off = [int(x) for x in offsets]
    return [mmr_row(items[off[b]:off[b + 1]], rel[off[b]:off[b + 1]], table, metric, lam, K, M, with_bound) for b in range(len(off) - 1)]


def stack(rows, field, dtype):
    return torch.tensor([row[field] for row in rows], dtype=dtype)
