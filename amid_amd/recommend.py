"""Top-K recommendations for every user of a CSV from saved weights (not in the reference, which only trains and evaluates).

Takes the model flags of ``train_sr.py`` (``--model --emb_dim --hid_dim --seq_len --bs --isItC --isInC --ts1 --ts2 -ds -dm
--overlap_ratio --data_root --device``; ``--isDR`` as in ``train_sr_dr.py``, here off unless given) and

    --weights FILE          best_d1.pt / best_d2.pt / a model.state_dict() (loaded strictly), or a last.pt (its training state)
    --users CSV             the rows to recommend for (default: the job's <dm>_test.csv)
    --topk K                1 .. 256
    --pool {dataset,table}  candidates: the two item pools of the job's training CSV, or every row of the table
    --history {eval,full}   eval: the rows as test() sees them (the last own-domain item held out as the positive);
                            full: that item appended again -- the recommendation after the whole history
    --out FILE.npz          user_id [N], domain_id [N], items [N, K] (CSV item ids, -1 where a pool ran out), scores [N, K], in CSV row order
    --metrics               also evaluate these weights with test() on the same CSV (sampled negatives, drop_last), printed and returned
    --vectors_out FILE.npz  also write the vector the scorer sees for every row of the CSV (SASRec.encode_users): user_id [N],
                            domain_id [N], vectors [N, D] -- the encode half of an encode-nightly / score-online split
    --similar_items {all | FILE}
                            instead of recommendations, write to --out the --topk nearest neighbours (--metric cosine | dot) in the
                            trained item table of every item of the candidate pools (all) or of the ids listed in FILE (text, or
                            .npy): item_id [M], neighbors [M, K] (-1 where the candidates ran out), scores [M, K].  The candidates are
                            --pool's: the union of the two dataset pools, or every row of the table
    --audience_of {all | FILE}
                            instead of recommendations, write to --out the audience of items (SASRec.recommend_users): the --topk rows of
                            --users that score the item highest, among the rows of the item's domain.  all: every item of the two
                            dataset pools (--pool dataset), each in its pool's domain; FILE: "item_id domain_id" pairs (text, or a .npy
                            array [M, 2]).  Written: item_id [M], domain_id [M], users [M, K] (the rows' user_id, -1 where the domain ran
                            out of rows), rows [M, K] (CSV row numbers), scores [M, K]
    --vectors_in FILE.npz   with --audience_of or --candidates: take the rows' vectors from a file --vectors_out wrote for the same CSV
                            instead of encoding them in this run
    --exclude_holders       with --audience_of: leave out of an item's audience every row whose own-domain history, the held-out item
                            included, contains the item
    --candidates FILE       instead of recommendations over a shared pool, rank each row's OWN candidate list
                            (SASRec.rank_candidates_from_vectors: an upstream retriever's output, an in-stock list, a hand-built negative
                            set).  FILE: an .npz with offsets [N + 1] and items [n] in the row order of --users (row r's list is
                            items[offsets[r] : offsets[r + 1]]; a user_id [N] array, if present, must equal the CSV's column), or a text
                            file with one line per CSV row, ids separated by whitespace or commas, an empty line an empty list.  Written:
                            user_id [N], domain_id [N], items [N, K] (-1 where the list ran out), scores [N, K], positions [N, K] (the
                            entry's index inside its row's list)
    --exclude_history       with --candidates: leave the ids of the row's own-domain sequence (under --history full the held-out item
                            too) out of its top-K.  Off by default: the list is the caller's
    --list_scores           with --candidates: also write offsets [N + 1], list_items [n] and list_scores [n], every entry's score
    --diversify LAMBDA      re-rank by greedy Maximal Marginal Relevance (SASRec.diversify; LAMBDA in 0 .. 1 weighs the relevance, --metric
                            is the item-item similarity): in the default mode over each row's top --shortlist of the same path, with
                            --candidates over each row's own list scored by the same path (--exclude_history leaves the history out,
                            --vectors_in as above).  --out gains mmr [N, K] (the criterion at each pick) and max_sim [N, K]; items and
                            scores keep their names, scores stays the relevance.  Not with --similar_items or --audience_of
    --shortlist M           with --diversify: how many of the best entries are re-ranked, --topk .. 256 (default min(256, max(topk, 100)))

    python recommend.py --data_root /path/to/AMID -ds amazon -dm cloth_sport --overlap_ratio 0.75 --model sasrec --bs 256 \
        --seq_len 50 --emb_dim 128 --weights runs/seed0/best_d1.pt --topk 10 --out cloth_sport_top10.npz
    python recommend.py ... --weights runs/seed0/best_d1.pt --vectors_out cloth_sport_users.npz
    python recommend.py ... --weights runs/seed0/best_d1.pt --similar_items all --metric cosine --topk 20 --out cloth_sport_similar.npz
    python recommend.py ... --weights runs/seed0/best_d1.pt --audience_of all --exclude_holders --topk 100 --out cloth_sport_audiences.npz
    python recommend.py ... --weights runs/seed0/best_d1.pt --candidates retrieved.npz --exclude_history --topk 20 --out cloth_sport_reranked.npz
    python recommend.py ... --weights runs/seed0/best_d1.pt --diversify 0.7 --shortlist 100 --topk 10 --out cloth_sport_diverse10.npz

Every row of the CSV gets a recommendation: the last batch is filled with rows from the start of the CSV (comp models need whole
``--bs``-row batches) and the surplus is cut off.  The ranking is ``SASRec.recommend_all``: one graph replay a batch.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import train_sr as base
from .dataset_seq import DeviceBatches, DualDomainSeqDataset
from .model_gru import GRU4Rec, GRU4RecAMID
from .model_seq import BERT4Rec, SASRec


def build_parser():
    p = base.build_parser()
    p.description = "Top-K recommendations from saved weights"
    p.add_argument("--isDR", type=bool, default=False, help="the weights are a doubly-robust model's (train_sr_dr.py)")
    p.add_argument("--weights", type=str, required=True, help="best_d1.pt / best_d2.pt / a state_dict, or a last.pt")
    p.add_argument("--users", type=str, default=None, help="CSV of the rows to recommend for (default: <data_root>/<ds>_dataset/<dm>_test.csv)")
    p.add_argument("--topk", type=int, default=10)
    p.add_argument("--pool", type=str, default="dataset", choices=("dataset", "table"))
    p.add_argument("--history", type=str, default="eval", choices=("eval", "full"))
    p.add_argument("--out", type=str, default="recommendations.npz")
    p.add_argument("--metrics", action="store_true", help="also run test() on the CSV with these weights")
    p.add_argument("--vectors_out", type=str, default=None, help="FILE.npz: also write user_id, domain_id and the scorer's vector of every row")
    p.add_argument("--similar_items", type=str, default=None, help="all | FILE of item ids: write their --topk nearest items to --out instead")
    p.add_argument("--metric", type=str, default="cosine", choices=("cosine", "dot"), help="the similarity of --similar_items")
    p.add_argument("--audience_of", type=str, default=None, help="all | FILE of 'item_id domain_id' pairs: write their --topk users to --out instead")
    p.add_argument("--vectors_in", type=str, default=None, help="FILE.npz that --vectors_out wrote for --users: the vectors --audience_of ranks")
    p.add_argument("--exclude_holders", action="store_true", help="--audience_of: leave out the rows whose history holds the item")
    p.add_argument("--candidates", type=str, default=None, help="FILE.npz (offsets, items) or text, a line a row: rank each row's own list to --out instead")
    p.add_argument("--exclude_history", action="store_true", help="--candidates: leave the row's own-domain history out of its top-K")
    p.add_argument("--list_scores", action="store_true", help="--candidates: also write the score of every entry of every list")
    p.add_argument("--diversify", type=float, default=None, metavar="LAMBDA",
                   help="re-rank by greedy MMR with this weight of the relevance, 0 .. 1 (top-K and --candidates; --metric is the similarity)")
    p.add_argument("--shortlist", type=int, default=None, metavar="M", help="--diversify: the best M entries are re-ranked (--topk .. 256)")
    return p


def check_diversify(args) -> None:
    """--diversify / --shortlist against the other flags: SystemExit before anything is loaded or written."""
    if args.diversify is None:
        if args.shortlist is not None:
            raise SystemExit("--shortlist belongs to --diversify")
        return
    if args.similar_items or args.audience_of:
        raise SystemExit("--diversify re-ranks recommendations (top-K or --candidates): not with --similar_items or --audience_of")
    if not 0.0 <= args.diversify <= 1.0:
        raise SystemExit(f"--diversify must be in 0..1, got {args.diversify}")
    if args.shortlist is not None and not args.topk <= args.shortlist <= 256:
        raise SystemExit(f"--shortlist must be in --topk..256 ({args.topk}..256), got {args.shortlist}")
    if args.shortlist is None:
        args.shortlist = min(256, max(args.topk, 100))


def diverse_fields(res) -> dict:
    """DiverseLists -> the arrays --diversify writes: items, scores (the relevance), mmr, max_sim [N, K]."""
    return {"items": res.ids.cpu().numpy(), "scores": res.scores.cpu().numpy(), "mmr": res.values.cpu().numpy(),
            "max_sim": res.max_sims.cpu().numpy()}


def full_history(seq_d1: np.ndarray, seq_d2: np.ndarray, i_node: np.ndarray, domain_id: np.ndarray):
    """--history full: every row's held-out item behind its own-domain sequence, the sequence shifted left by one (its oldest entry,
    a pad id where the history is short, drops out); the other domain's sequence is unchanged.  [N, T] int64 arrays in, copies out."""
    s1, s2 = seq_d1.copy(), seq_d2.copy()
    for s, rows in ((s1, domain_id == 0), (s2, domain_id != 0)):
        s[rows, :-1] = s[rows, 1:]
        s[rows, -1] = i_node[rows]
    return s1, s2


def filled_batches(n_rows: int, bs: int) -> np.ndarray:
    """Row indices [n_batches, bs] covering 0 .. n_rows - 1 in order; the last batch's tail is rows from the start again."""
    nb = (n_rows + bs - 1) // bs
    return (np.arange(nb * bs) % n_rows).reshape(nb, bs)


def listed_ids(path: str) -> np.ndarray:
    """--similar_items FILE: the item ids of a .npy array or of a text file (whitespace or commas between them)."""
    if path.endswith(".npy"):
        return np.load(path).astype(np.int64).reshape(-1)
    with open(path) as f:
        return np.array([int(x) for x in f.read().replace(",", " ").split()], dtype=np.int64)


def write_npz(path: str, out) -> None:
    if os.path.dirname(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez(path, **out)


def similar_items_main(model, args, pool) -> dict:
    """--similar_items: the neighbours of the pools' items (or the listed ones) among --pool's candidates, to --out."""
    dev = torch.device(args.device)
    cand = None if pool is None else torch.unique(torch.cat(pool))
    if args.similar_items == "all":
        items = cand if cand is not None else torch.arange(model.engine.n_rows, dtype=torch.int64, device=dev)
    else:
        items = torch.from_numpy(listed_ids(args.similar_items)).to(dev)
        if items.numel() < 1:
            raise SystemExit(f"{args.similar_items}: no item ids")
    ids, scores = model.similar_items(items, k=args.topk, metric=args.metric, pool=cand)
    out = {"item_id": items.cpu().numpy(), "neighbors": ids.cpu().numpy(), "scores": scores.cpu().numpy()}
    write_npz(args.out, out)
    print(f"wrote {args.out}: the {args.topk} nearest items ({args.metric}) of {items.numel()} items")
    return out


def listed_items(path: str):
    """--audience_of FILE: (item ids, domain ids) of a .npy array [M, 2] or of a text file of "item_id domain_id" pairs (whitespace or
    commas between the numbers)."""
    if path.endswith(".npy"):
        flat = np.load(path).astype(np.int64).reshape(-1)
    else:
        flat = listed_ids(path)
    if flat.size < 2 or flat.size % 2:
        raise SystemExit(f"{path}: expected 'item_id domain_id' pairs")
    pairs = flat.reshape(-1, 2)
    if not np.isin(pairs[:, 1], (0, 1)).all():
        raise SystemExit(f"{path}: a domain_id is 0 or 1")
    return pairs[:, 0].copy(), pairs[:, 1].copy()


def holders_of(items: np.ndarray, item_dom: np.ndarray, seq_d1: np.ndarray, seq_d2: np.ndarray, i_node: np.ndarray, domain_id: np.ndarray):
    """--exclude_holders: for each query (item, domain) the rows of that domain whose own-domain sequence or held-out item is the item,
    as recommend_users' (indices, offsets [M + 1]) -- ascending rows, a row once per occurrence."""
    d = (domain_id != 0).astype(np.int64)
    own = np.concatenate((np.where(d[:, None] != 0, seq_d2, seq_d1), i_node[:, None]), axis=1).astype(np.int64)
    key = (own * 2 + d[:, None]).reshape(-1)
    rows = np.repeat(np.arange(own.shape[0], dtype=np.int64), own.shape[1])
    order = np.argsort(key, kind="stable")
    key, rows = key[order], rows[order]
    qk = items.astype(np.int64) * 2 + (item_dom != 0)
    lo, hi = np.searchsorted(key, qk, "left"), np.searchsorted(key, qk, "right")
    offsets = np.zeros(len(qk) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(hi - lo)
    take = np.repeat(lo - offsets[:-1], hi - lo) + np.arange(offsets[-1], dtype=np.int64)
    return rows[take], offsets


def load_vectors(args, ds) -> torch.Tensor:
    """--vectors_in: the vectors [N, D] of a file --vectors_out wrote for this CSV, on the device; SystemExit if it is another CSV's."""
    N = len(ds)
    with np.load(args.vectors_in) as f:
        if not {"user_id", "domain_id", "vectors"} <= set(f.files):
            raise SystemExit(f"{args.vectors_in}: not a file --vectors_out wrote (user_id, domain_id, vectors)")
        uid, dom_in, vec = f["user_id"], f["domain_id"], f["vectors"]
    if vec.ndim != 2 or vec.shape[0] != N or uid.shape != (N,) or not np.array_equal(uid, ds.user_nodes) \
            or not np.array_equal(dom_in, ds.domain_id):
        raise SystemExit(f"{args.vectors_in} does not match the users CSV: it holds {vec.shape[0]} rows, the CSV {N}; the row count, "
                         f"the user_id column and the domain_id column must be the CSV's")
    if vec.shape[1] != args.emb_dim:
        raise SystemExit(f"{args.vectors_in}: vectors of {vec.shape[1]} elements, --emb_dim is {args.emb_dim}")
    return torch.from_numpy(np.ascontiguousarray(vec, dtype=np.float32)).to(torch.device(args.device))


def candidate_lists(path: str, n_rows: int, user_ids: np.ndarray):
    """--candidates FILE as (items int64 [n], offsets int64 [n_rows + 1]): an .npz with `offsets` and `items` (and optionally `user_id`,
    which must be the CSV's column), or a text file with one line per CSV row (ids separated by whitespace or commas; an empty line is an
    empty list).  SystemExit where the file does not fit the CSV's n_rows rows."""
    if path.endswith(".npz"):
        with np.load(path) as f:
            if not {"offsets", "items"} <= set(f.files):
                raise SystemExit(f"{path}: expected the arrays offsets [N + 1] and items [n]")
            offsets, items = f["offsets"].astype(np.int64).reshape(-1), f["items"].astype(np.int64).reshape(-1)
            uid = f["user_id"] if "user_id" in f.files else None
    else:
        with open(path) as f:
            lines = f.read().split("\n")
        if lines and lines[-1] == "":
            lines.pop()                                                                    # (the newline that ends the last row)
        rows = [[int(x) for x in ln.replace(",", " ").split()] for ln in lines]
        offsets = np.zeros(len(rows) + 1, dtype=np.int64)
        offsets[1:] = np.cumsum([len(r) for r in rows])
        items = np.array([x for r in rows for x in r], dtype=np.int64)
        uid = None
    if offsets.size != n_rows + 1:
        raise SystemExit(f"{path} holds the lists of {max(offsets.size - 1, 0)} rows, the users CSV has {n_rows}")
    if offsets[0] != 0 or offsets[-1] != items.size or (np.diff(offsets) < 0).any():
        raise SystemExit(f"{path}: offsets must rise from 0 to the number of items ({items.size})")
    if uid is not None and (uid.shape != (n_rows,) or not np.array_equal(uid, user_ids)):
        raise SystemExit(f"{path} does not match the users CSV: its user_id array is not the CSV's user_id column")
    return items, offsets


def candidates_main(model, args, ds, vectors, history) -> dict:
    """--candidates: the --topk best entries of each row's own list, to --out.  vectors: the rows' vectors [N, D] on the device;
    history: [N, T] ids to leave out (--exclude_history) or None."""
    dev = torch.device(args.device)
    N = len(ds)
    items, offsets = candidate_lists(args.candidates, N, ds.user_nodes)
    lists = (torch.from_numpy(items).to(dev), torch.from_numpy(offsets))
    out = {"user_id": ds.user_nodes.copy(), "domain_id": ds.domain_id.copy()}
    if args.diversify is None:
        res = model.rank_candidates_from_vectors(vectors, torch.from_numpy(ds.domain_id).to(dev), lists, k=args.topk, history=history,
                                                 list_scores=args.list_scores)
        out.update(items=res.ids.cpu().numpy(), scores=res.scores.cpu().numpy())
    else:
        # every entry's score from the same path, then MMR over each list; an entry of the row's history is absent (NaN relevance)
        scored = model.rank_candidates_from_vectors(vectors, torch.from_numpy(ds.domain_id).to(dev), lists, k=None, list_scores=True)
        rel = scored.list_scores
        if history is not None:
            rel = rel.clone()
            row = torch.repeat_interleave(torch.arange(N, device=dev), torch.from_numpy(np.diff(offsets)).to(dev))
            for e0 in range(0, items.size, 1 << 18):
                e = slice(e0, e0 + (1 << 18))
                rel[e] = torch.where((history[row[e]] == lists[0][e].unsqueeze(1)).any(1), torch.full_like(rel[e], float("nan")), rel[e])
        res = model.diversify(lists, rel, k=args.topk, lam=args.diversify, metric=args.metric, shortlist=args.shortlist)
        out.update(diverse_fields(res))
        res = scored._replace(positions=res.positions)
    out["positions"] = res.positions.cpu().numpy()
    if args.list_scores:
        out.update(offsets=offsets, list_items=items, list_scores=res.list_scores.cpu().numpy())
    write_npz(args.out, out)
    print(f"wrote {args.out}: top-{args.topk} of the own lists of {N} rows ({items.size} candidates)"
          + (", histories left out" if args.exclude_history else "")
          + (f", diversified (lambda {args.diversify}, {args.metric}) over the best {args.shortlist}" if args.diversify is not None else ""))
    return out


def audience_main(model, args, ds, pool, vectors) -> dict:
    """--audience_of: the --topk rows of the CSV that score each listed item (or each item of the two dataset pools) highest, to --out.
    vectors: this run's encode_users rows [N, D] on the device, or None with --vectors_in."""
    dev = torch.device(args.device)
    N = len(ds)
    if args.vectors_in:
        vectors = load_vectors(args, ds)
    if args.audience_of == "all":
        if pool is None:
            raise SystemExit("--audience_of all takes the items of the two dataset pools: use --pool dataset, or list the items in a FILE")
        items = torch.cat(pool)
        item_dom = torch.cat((torch.zeros_like(pool[0]), torch.ones_like(pool[1])))
    else:
        it, dm = listed_items(args.audience_of)
        items, item_dom = torch.from_numpy(it).to(dev), torch.from_numpy(dm).to(dev)
    holders = None
    if args.exclude_holders:
        idx, off = holders_of(items.cpu().numpy(), item_dom.cpu().numpy(), ds.seq_d1, ds.seq_d2, ds.i_node, ds.domain_id)
        holders = (torch.from_numpy(idx).to(dev), torch.from_numpy(off).to(dev))
    rows, scores = model.recommend_users(items, item_dom, vectors, torch.from_numpy(ds.domain_id).to(dev), k=args.topk, holders=holders)
    rows = rows.cpu().numpy()
    users = np.where(rows >= 0, ds.user_nodes[np.maximum(rows, 0)], -1)
    out = {"item_id": items.cpu().numpy(), "domain_id": item_dom.cpu().numpy(), "users": users, "rows": rows, "scores": scores.cpu().numpy()}
    write_npz(args.out, out)
    print(f"wrote {args.out}: the {args.topk} best of {N} rows for {items.numel()} items"
          + (", holders left out" if args.exclude_holders else ""))
    return out


def load_weights(model, path: str) -> str:
    """Load `path` into the model; returns what it was ("training state" / "state dict")."""
    ck = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(ck, dict) and "format" in ck and "engine" in ck:
        model.load_training_state(ck)
        return "training state"
    model.load_state_dict(ck, strict=True)
    return "state dict"


def main(argv=None):
    args = build_parser().parse_args(argv)
    if "+" in args.domain_type:
        raise SystemExit(f"recommend.py with a joint job (-dm {args.domain_type}) is not supported: recommend for one dataset per run")
    if not 1 <= args.topk <= 256:
        raise SystemExit(f"--topk must be in 1..256, got {args.topk}")
    if args.audience_of and args.similar_items:
        raise SystemExit("--audience_of and --similar_items both write --out: one of them per run")
    if args.candidates and (args.audience_of or args.similar_items):
        raise SystemExit("--candidates, --audience_of and --similar_items all write --out: one of them per run")
    if args.exclude_holders and not args.audience_of:
        raise SystemExit("--exclude_holders belongs to --audience_of")
    if args.vectors_in and not (args.audience_of or args.candidates):
        raise SystemExit("--vectors_in belongs to --audience_of or --candidates")
    if (args.exclude_history or args.list_scores) and not args.candidates:
        raise SystemExit("--exclude_history and --list_scores belong to --candidates")
    check_diversify(args)
    base.check_neg_sampling(args)
    cls ={"gru4rec": GRU4Rec, "sasrec": SASRec, "bert4rec": BERT4Rec}.get(args.model.lower())
    if cls is None:
        raise SystemExit(f"unknown --model {args.model!r} (gru4rec | sasrec | bert4rec)")
    if cls is GRU4Rec and (args.isInC or args.isItC or args.isDR):
        cls = GRU4RecAMID                                                                  # (the plain class refuses the flags: model_gru.py)
    user_length, item_length = 895510, 447410                                             # train_sr.py:447, :450
    root = os.path.join(args.data_root, f"{args.dataset_type}_dataset")
    users_csv = args.users or os.path.join(root, f"{args.domain_type}_test.csv")
    ds = DualDomainSeqDataset(seq_len=args.seq_len, isTrain=False, neg_nums=args.neg_nums, long_length=args.long_length,
                              pad_id=item_length + 1, seed=1000, csv_path=users_csv)
    if len(ds) < 1:
        raise SystemExit(f"{users_csv}: no rows")
    torch.cuda.set_device(torch.device(args.device))
    model = cls(user_length=2 * user_length, user_emb_dim=args.emb_dim, item_length=2 * item_length, item_emb_dim=args.emb_dim,
                seq_len=args.seq_len, hid_dim=args.hid_dim, bs=args.bs, isInC=args.isInC, isItC=args.isItC, threshold1=args.ts1,
                threshold2=args.ts2, isDR=bool(args.isDR), seed=0)
    kind = load_weights(model, args.weights)
    model.eval()
    print(f"{args.weights}: {kind}; {len(ds)} rows of {users_csv}")
    dev = torch.device(args.device)
    pool = None
    neg_eval = args.metrics and args.neg_sampling == "popularity" and args.neg_sampling_for in ("both", "eval")
    if args.pool == "dataset" or neg_eval:
        train_csv = os.path.join(root, f"{args.domain_type}_train{int(args.overlap_ratio * 100)}.csv")
        ds_train = DualDomainSeqDataset(seq_len=args.seq_len, isTrain=True, neg_nums=1, long_length=args.long_length, pad_id=item_length + 1,
                                        seed=0, csv_path=train_csv)
        if args.pool == "dataset":
            pool = tuple(torch.from_numpy(p).to(dev) for p in ds_train.pool)              # sorted unique (dataset_seq.py:141-142)
    s1, s2 = ds.seq_d1, ds.seq_d2
    if args.history == "full":
        s1, s2 = full_history(s1, s2, ds.i_node, ds.domain_id)
    sel = filled_batches(len(ds), args.bs)
    users = {"seq_d1": torch.from_numpy(s1[sel]).to(dev), "seq_d2": torch.from_numpy(s2[sel]).to(dev),
             "domain_id": torch.from_numpy(ds.domain_id[sel]).to(dev)}
    N = len(ds)
    vectors = None
    if args.audience_of or args.candidates:
        enc = None
        if args.vectors_out or not args.vectors_in:
            enc = model.encode_users(users, use_graph=not args.no_graph).reshape(-1, args.emb_dim)[:N]
        if args.vectors_out:
            vectors = enc.cpu().numpy()
            write_npz(args.vectors_out, {"user_id": ds.user_nodes.copy(), "domain_id": ds.domain_id.copy(), "vectors": vectors})
            print(f"wrote {args.vectors_out}: the scorer's vectors of {N} rows")
        if args.candidates:
            history = torch.from_numpy(np.where(ds.domain_id[:, None] != 0, s2, s1)).to(dev) if args.exclude_history else None
            out = candidates_main(model, args, ds, load_vectors(args, ds) if args.vectors_in else enc, history)
        else:
            out = audience_main(model, args, ds, pool, enc)
        if vectors is not None:
            out["vectors"] = vectors
        return out
    if args.vectors_out:
        vectors = model.encode_users(users, use_graph=not args.no_graph).reshape(-1, args.emb_dim)[:N].cpu().numpy()
        write_npz(args.vectors_out, {"user_id": ds.user_nodes.copy(), "domain_id": ds.domain_id.copy(), "vectors": vectors})
        print(f"wrote {args.vectors_out}: the scorer's vectors of {N} rows")
    if args.similar_items:
        out = similar_items_main(model, args, pool)
        if vectors is not None:
            out["vectors"] = vectors
        return out
    kk = args.topk if args.diversify is None else args.shortlist       # (--diversify: the shortlist is the top-M of the same path)
    ids, scores = model.recommend_all(users, k=kk, pool=pool, exclude_history=True, use_graph=not args.no_graph)
    out = {"user_id": ds.user_nodes.copy(), "domain_id": ds.domain_id.copy()}
    if args.diversify is None:
        out.update(items=ids.reshape(-1, kk)[:N].cpu().numpy(), scores=scores.reshape(-1, kk)[:N].cpu().numpy())
    else:
        out.update(diverse_fields(model.diversify_ranked(ids.reshape(-1, kk)[:N], scores.reshape(-1, kk)[:N], k=args.topk, lam=args.diversify,
                                                         metric=args.metric)))
    if os.path.dirname(args.out):
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
    np.savez(args.out, **out)
    print(f"wrote {args.out}: top-{args.topk} of {N} rows ({sel.shape[0]} batches of {args.bs})"
          + (f", diversified (lambda {args.diversify}, {args.metric}) over the top {kk}" if args.diversify is not None else ""))
    if vectors is not None:
        out["vectors"] = vectors
    out["metrics"] = None
    if args.metrics:
        val = DeviceBatches(ds, args.bs, shuffle=False, device=args.device, seed=0,
                            **(base.neg_loader_args(args, "eval", ds, ds_train) if neg_eval else {}))
        res = base.test(model, args, val)
        names = ("HR@1", "NDCG@1", "HR@5", "NDCG@5", "HR@10", "NDCG@10", "MRR")
        for key, sc in res.items():
            print(f"val {key}: " + (f"{sc:.4f}" if key == "loss" else ", ".join(f"{n}: {v:.4f}" for n, v in zip(names, sc))))
        out["metrics"] = res
    return out


if __name__ == "__main__":
    main()
