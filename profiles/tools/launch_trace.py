"""The launches of one eager step of each driver path, as text: what every C-ABI call was given.  Two trees that print the same traces
hand the same arguments to the same entry points in the same order -- the check of a change to HOW the driver passes arguments
(profiles/launch_trace.md).

One line per launch: the entry name, then every argument.  A scalar is printed by value; a pointer as the ordinal of its first appearance in
the scenario's trace (null = 0), so the line does not depend on where the allocator put things; a host pointer array element by element, a
host int array by its values.  Nothing but lib().timer (the hook bench.py's KernelTimer uses), the engines' public methods and -- for the
data-parallel local half in one process -- the _tail_pack attribute engine_dp sets around graph A is used, so the file runs unchanged
against another tree's amid_amd/*.py (AMID_TREE) on the same library (AMID_LIB_PATH).

    python profiles/tools/launch_trace.py --out DIR           every scenario, each in a child process under its own time limit (the first
                                                              abnormal exit ends the run), then the coverage check and the table
    python profiles/tools/launch_trace.py --out DIR --dry     ... in this process, recording the calls WITHOUT launching them
    python profiles/tools/launch_trace.py --scenario NAME     one scenario's trace on stdout
"""
import argparse, ctypes, fnmatch, hashlib, os, re, subprocess, sys
ROOT = os.environ.get("AMID_TREE", os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def entries_bound_by_name():
    """Every entry point a call_named site of THIS tree's drivers names (amid_amd/engine*.py), read from the sources: string constants, the
    branches of a conditional, and f-strings whose holes are names assigned string constants in the same function (a hole that is anything
    else -- a plan's row-tile suffix -- is a "*": any declared entry that fits).  Each must be launched by at least one scenario."""
    import ast, fnmatch, glob, itertools
    declared = set(re.findall(r"\b(amid_\w+)\s*\(", open(os.path.join(HERE, "include", "amid_hip.h")).read()))

    def values(node, fn):
        if isinstance(node, ast.Constant) and isinstance(node.value, str):
            return [node.value]
        if isinstance(node, ast.IfExp):
            return values(node.body, fn) + values(node.orelse, fn)
        if isinstance(node, ast.BinOp) and isinstance(node.op, ast.Add):
            return [a + b for a in values(node.left, fn) for b in values(node.right, fn)]
        if isinstance(node, ast.JoinedStr):
            parts = [values(v.value if isinstance(v, ast.FormattedValue) else v, fn) for v in node.values]
            return ["".join(c) for c in itertools.product(*parts)]
        if isinstance(node, ast.Name):          # what the enclosing function assigns to the name, tuple assignments element by element
            out = []
            for a in (n for n in ast.walk(fn) if isinstance(n, ast.Assign)):
                for t in a.targets:
                    if isinstance(t, ast.Name) and t.id == node.id:
                        out += values(a.value, fn)
                    elif isinstance(t, ast.Tuple):
                        for i, e in enumerate(t.elts):
                            if isinstance(e, ast.Name) and e.id == node.id:
                                srcs = [a.value.body, a.value.orelse] if isinstance(a.value, ast.IfExp) else [a.value]
                                out += [v for src in srcs if isinstance(src, ast.Tuple) for v in values(src.elts[i], fn)]
            return out or ["*"]
        return ["*"]

    found = set()
    for path in sorted(glob.glob(os.path.join(HERE, "amid_amd", "engine*.py"))):
        tree = ast.parse(open(path).read())
        scopes = tree.body + [n for c in tree.body if isinstance(c, ast.ClassDef) for n in c.body]
        for fn in (n for n in scopes if isinstance(n, ast.FunctionDef)):          # (a method with its nested functions: one scope of names)
            for c in (n for n in ast.walk(fn) if isinstance(n, ast.Call)):
                if isinstance(c.func, ast.Attribute) and c.func.attr == "call_named" and c.args:
                    names = set(values(c.args[0], fn))
                    unknown = {n for n in names if not fnmatch.filter(declared, n)}
                    assert names and not unknown, f"{path}:{c.lineno}: call_named names {sorted(unknown) or 'nothing the tool can read'}"
                    found |= names
    return sorted(found)


N_ITEMS, FIX = 3000, 1e-7


def pointer_params():
    """entry -> per parameter: is it a pointer (the header's own declarations)."""
    text = open(os.path.join(ROOT, "include", "amid_hip.h")).read()
    text = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    return {m.group(1): ["*" in a for a in m.group(2).split(",")] for m in re.finditer(r"\b(amid_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S)}


class Tracer:
    """lib().timer: prints the call, then launches it (dry: does not)."""

    def __init__(self, dry):
        self.dry, self.is_ptr, self.lines, self.seen = dry, pointer_params(), [], {}

    def ordinal(self, p):
        p = getattr(p, "value", p) or 0
        return 0 if not p else self.seen.setdefault(int(p), len(self.seen) + 1)

    def show(self, a, is_ptr):
        if isinstance(a, ctypes.Array):
            if a._type_ is ctypes.c_void_p:
                return "[" + " ".join(f"@{self.ordinal(p)}" for p in a) + "]"
            return "[" + " ".join(repr(v) for v in a) + "]"
        return f"@{self.ordinal(a)}" if is_ptr else repr(a)

    def timed_call(self, L, name, args):
        kinds = self.is_ptr[name]
        assert len(kinds) == len(args), (name, len(kinds), len(args))
        self.lines.append(name + " " + " ".join(self.show(a, k) for a, k in zip(args, kinds)))
        if self.dry:
            return
        code = L._fn[name](*args)
        if code != 0:
            raise RuntimeError(f"{name} returned {code}")


def sasrec(D=128, T=20, B=32, NI=2, compute="f32", need_grad=True, hid=32, **variant):
    import torch
    from oracle import amid_oracle as orc
    from amid_amd.engine import SasrecEngine
    kw = dict(itc_bs=B if variant.get("itc") else 0, inc_bs=B if variant.get("inc") else 0, dr=bool(variant.get("dr")))
    eng = SasrecEngine(N_ITEMS, D, T, hid, lr=1e-3, seed=5, compute=compute, **kw)
    eng.load_state_dict(orc.random_params(orc.sasrec_param_shapes(N_ITEMS, D, T, hid, **kw), seed=3))
    pl = eng.plan(B, T, NI, need_grad=need_grad)
    b = {k: v.cuda() for k, v in orc.synthetic_batch(B, T, N_ITEMS - 1, pad_id=N_ITEMS - 1, neg=NI - 1, seed=7).items()}
    return eng, pl, b, (torch.ones_like(b["domain_id"]) if kw["dr"] else None)


def bert(T=20, B=32, NI=2, need_grad=True, hid=32):
    from oracle import amid_oracle as orc
    from amid_amd.engine_bert import Bert4recEngine
    eng = Bert4recEngine(N_ITEMS, orc.BERT_HIDDEN, T, hid, lr=5e-4, seed=0)
    eng.load_state_dict(orc.random_params(orc.bert4rec_param_shapes(N_ITEMS, hid), seed=3))
    pl = eng.plan(B, T, NI, need_grad=need_grad)
    b = {k: v.cuda() for k, v in orc.synthetic_batch(B, T, N_ITEMS - 1, pad_id=0, neg=NI - 1, seed=7).items()}
    return eng, pl, b, None


def load(eng, pl, b, ob, pool=False):
    import torch
    args = (b["i_node"], b["neg_samples"], b["seq_d1"], b["seq_d2"], b["label"], b["domain_id"])
    if pool:
        eng.set_input_pool(pl, torch.stack([eng.pack_batch(pl, *args)] * 2))
    else:
        eng.load_batch(pl, *args, ob)


def train(make=sasrec, pool=False, **kw):
    def run():
        eng, pl, b, ob = make(**kw)
        load(eng, pl, b, ob, pool)
        return eng, lambda: eng.enqueue_train_step(pl)
    return run


def local_grads(pack=False, dense=True, pool=True, **kw):
    """The data-parallel step's local half in one process (a world of one): enqueue_local_grads -- pack: with graph A's packing tail --, then
    the optimizer over the gathered chunks (pack) or over the lists an eager exchange hands back."""
    def run():
        eng, pl, b, ob = sasrec(**kw)
        load(eng, pl, b, ob, pool)
        umax = eng.n_sparse_train(pl, dp=True)
        be = eng.merge_backend(umax)
        dgrad = eng.dense.grad if dense else None

        def step():
            if not pack:
                eng.enqueue_local_grads(pl)
                eng.enqueue_optimizer(pl, sparse=(pl.uniq_ids, pl.uniq_grad, pl.n_uniq))
                return
            eng._tail_pack = (be.send[: be.chunk_rows(umax, dgrad) * eng.D], umax, dense)
            try:
                eng.enqueue_local_grads(pl)
            finally:
                eng._tail_pack = None
            eng.enqueue_optimizer_gathered(be, be.gather_buffer(1, umax, dense=dgrad), 1, umax, dense_in_chunk=dense)
        return eng, step
    return run


def loop(clip=False, **kw):
    """The reference's own loop on the engine (amid_amd/optim.py): forward, backward, then the loop optimizer on a gradient buffer of the caller's."""
    def run():
        import torch
        eng, pl, b, ob = sasrec(**kw)
        load(eng, pl, b, ob)
        g, sq = torch.zeros_like(eng.dense.grad), torch.zeros(1, dtype=torch.float32, device=eng.device)

        def step():
            eng.enqueue_prepare(pl, sparse=True)
            eng.enqueue_forward(pl, train=True, with_loss=True)
            eng.enqueue_backward(pl, train=True)
            if clip:
                eng.enqueue_grad_sqnorm(pl, g, sq)
                eng.enqueue_loop_optimizer(pl, g, sq, 1.0)
            else:
                eng.enqueue_loop_optimizer(pl, g)
        return eng, step
    return run


def catalog(kind, **kw):
    """The full-catalog launches on a loaded batch: every row's positive ranked against its domain's whole pool, the pools' k best, and
    the k best for vectors of the caller's."""
    def run():
        import torch
        eng, pl, b, ob = sasrec(NI=5, need_grad=False, **kw)
        load(eng, pl, b, ob)
        B, k, dev = pl.shape.B, 10, eng.device
        pools = tuple(torch.arange(lo, hi, dtype=torch.int64, device=dev) for lo, hi in ((0, N_ITEMS // 2), (N_ITEMS // 2, N_ITEMS - 1)))
        dom, pos = b["domain_id"].reshape(-1), b["i_node"].reshape(-1)
        rank, rank_raw = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(2))
        ids, scores = torch.zeros(B, k, dtype=torch.int64, device=dev), torch.zeros(B, k, dtype=torch.float32, device=dev)
        u = torch.zeros(B, eng.D, dtype=torch.float32, device=dev)
        step = {"full_rank": lambda: eng.enqueue_full_rank(pl, pos, dom, pools, None, None, None, FIX, rank, rank_raw),
                "topk": lambda: eng.enqueue_topk(pl, dom, pools, None, None, None, k, False, ids, scores),
                "topk_vectors": lambda: eng.enqueue_topk_vectors(u, dom, pools, None, k, ids, scores, eng.flags_holder().err)}[kind]
        return eng, step
    return run


def evaluate(make=sasrec, NI=5, **kw):
    def run():
        eng, pl, b, ob = make(NI=NI, need_grad=False, **kw)
        load(eng, pl, b, ob)
        return eng, lambda: eng.enqueue_eval(pl, FIX, with_loss=True, want_scores=True)
    return run


def forward(make=sasrec, **kw):
    """model.forward's launches: both domains of every row, the candidates gathered by K1, the head as a launch of its own."""
    def run():
        eng, pl, b, ob = make(need_grad=False, **kw)
        load(eng, pl, b, ob)
        return eng, lambda: (eng.enqueue_prepare(pl, sparse=False), eng.enqueue_forward(pl, train=False, with_loss=False))
    return run


# name -> (class switches flipped for the scenario, its builder).  Shapes: the smallest of the tests' tables that reach each branch.
SCENARIOS = {}
for c in ("f32", "bf16"):          # the folded step on an input pool (16 < T: the head may ride on the forward)
    for g in (True, False):
        for h in (True, False):
            SCENARIOS[f"fold_{c}_gather{int(g)}_head{int(h)}"] = (dict(GATHER_ON_FWD=g, HEAD_ON_FWD=h), train(pool=True, compute=c, B=64))
SCENARIOS.update({
    "fold_t50": ({}, train(pool=True, T=50, B=37)),
    "unfolded_d128": ({}, train()),                                   # T <= 32: the one-launch backward
    "unfolded_d64": ({}, train(D=64, hid=16)),
    "unfolded_bf16": ({}, train(compute="bf16")),
    "unfolded_t13": ({}, train(T=13)),
    "unfolded_t32_d64": ({}, train(T=32, D=64, hid=16, B=64)),
    "strips_t50": ({}, train(T=50)),                                  # 32 < T, B <= n_CU: the five strip launches
    "strips_t50_d64": ({}, train(T=50, D=64, hid=16)),
    "seq_backward_t50": (dict(SEQ_BACKWARD="1"), train(T=50)),
    "head_own_launches": (dict(FUSED_HEAD=False), train()),
    "row_tiles": (dict(STRIP_KERNELS=False, FUSED_HEAD=False), train(T=16)),
    "itc_dr": ({}, train(itc=True, dr=True)),
    "inc": ({}, train(inc=True, T=16)),
    "eval_plain": ({}, evaluate()),
    "eval_plain_own_gather": (dict(GATHER_ON_FWD=False), evaluate()),
    "eval_d64": ({}, evaluate(D=64, hid=16)),
    "eval_bf16": ({}, evaluate(compute="bf16")),
    "eval_dr": ({}, evaluate(dr=True)),
    "eval_itc": ({}, evaluate(itc=True)),
    "eval_inc": ({}, evaluate(inc=True, T=16)),
    "eval_long": ({}, evaluate(T=80)),
    "eval_long_itc": ({}, evaluate(T=80, itc=True)),
    "forward_plain": ({}, forward()),
    "bert_eval": ({}, evaluate(make=bert)),
    "bert_forward": ({}, forward(make=bert)),
    "bert_head_own_launches": (dict(FUSED_HEAD=False), train(make=bert)),
    # ---- the forms the step takes with a switch off, and the drivers beside enqueue_train_step
    "fold_unprepared": (dict(PREPARED_POOL=False), train(pool=True, B=64)),             # riders on the strips and the weight gradients
    "fold_unprepared_t50": (dict(PREPARED_POOL=False), train(pool=True, T=50, B=37)),
    "fold_no_fused_opt": (dict(FUSED_OPT=False), train(pool=True, B=64)),               # the tail and the optimizer as launches of their own
    "fold_no_fused_opt_unprepared": (dict(FUSED_OPT=False, PREPARED_POOL=False), train(pool=True, B=64)),
    "fold_fwd_unsplit": (dict(FWD_SPLIT=False), train(pool=True, B=64)),                # the folded tail behind a forward that saved qn / y
    "fold_fwd_unsplit_unprepared": (dict(FWD_SPLIT=False, PREPARED_POOL=False), train(pool=True, B=64)),
    "pool_no_fused_tail": (dict(FUSED_TAIL=False), train(pool=True, B=64)),             # round 4's sequence on a pool
    "pool_no_fused_tail_t50": (dict(FUSED_TAIL=False), train(pool=True, T=50, B=37)),
    "pool_d64": ({}, train(pool=True, D=64, hid=16)),
    "no_fused_opt": (dict(FUSED_OPT=False), train()),
    "no_fused_opt_t50": (dict(FUSED_OPT=False), train(T=50)),
    "no_fused_spans": (dict(FUSED_SPANS=False), train()),
    "no_fused_spans_t50": (dict(FUSED_SPANS=False), train(T=50)),
    "fold_catchup": (dict(FOLD_CATCHUP="1"), train()),
    "fold_catchup_t50": (dict(FOLD_CATCHUP="1"), train(T=50)),
    "fold_catchup_pool": (dict(FOLD_CATCHUP="1"), train(pool=True, B=64)),
    "sort_chain": (dict(SORT_CHAIN=True), train()),
    "sort_chain_pool": (dict(SORT_CHAIN=True), train(pool=True, D=64, hid=16)),
    "no_sort_riders_t50": (dict(SORT_RIDERS=False), train(T=50)),
    "row_tiles_live": (dict(STRIP_KERNELS=False), train(T=16)),
    "row_tiles_t50": (dict(STRIP_KERNELS=False), train(T=50, D=64, hid=16)),
    "row_tiles_itc": (dict(STRIP_KERNELS=False), train(itc=True, T=16)),                 # every sequence carries a gradient: the forms without a row list
    "pool_itc": ({}, train(pool=True, itc=True)),                                       # a pool batch without a live list
    "compact_live": (dict(COMPACT_MIN_IDX=0), train(T=50)),                             # K1 writes the compact index list
    "compact_live_fwd_unsplit": (dict(COMPACT_MIN_IDX=0, FWD_SPLIT=False), train(T=50)),
    "compact_live_pool": (dict(COMPACT_MIN_IDX=0, FUSED_TAIL=False), train(pool=True, T=50, B=37)),
    "strips_forward_t50": (dict(SEQ_FORWARD=False), train(T=50)),                       # the forward as strip launches
    "strips_forward_bf16": (dict(SEQ_FORWARD=False), train(T=50, compute="bf16")),
    "dp_fold": ({}, local_grads(B=64)),
    "dp_fold_pack": ({}, local_grads(pack=True, B=64)),
    "dp_fold_pack_sparse_only": ({}, local_grads(pack=True, dense=False, B=64)),
    "dp_fold_no_fused_opt": (dict(FUSED_OPT=False), local_grads(B=64)),
    "dp_fold_no_fused_opt_pack": (dict(FUSED_OPT=False), local_grads(pack=True, B=64)),
    "dp_fold_no_fused_opt_pack_sparse_only": (dict(FUSED_OPT=False), local_grads(pack=True, dense=False, B=64)),
    "dp_fold_unprepared_pack": (dict(PREPARED_POOL=False), local_grads(pack=True, B=64)),
    "dp_plain": ({}, local_grads(pool=False)),
    "dp_plain_pack": ({}, local_grads(pack=True, pool=False)),
    "dp_plain_pack_t50": ({}, local_grads(pack=True, dense=False, pool=False, T=50)),
    "full_rank": ({}, catalog("full_rank")),
    "topk": ({}, catalog("topk")),
    "topk_vectors": ({}, catalog("topk_vectors")),
    "loop_optimizer": ({}, loop()),
    "loop_optimizer_clip": ({}, loop(clip=True, T=50)),
    "bert_train": ({}, train(make=bert)),
    "bert_train_t50": ({}, train(make=bert, T=50)),
    "bert_train_fp32_strips": (dict(STRIP_P3=False), train(make=bert)),
    "bert_train_row_tiles": (dict(STRIP_KERNELS=False), train(make=bert)),
    "bert_train_pool": ({}, train(make=bert, pool=True)),
})


def trace(name, dry):
    from amid_amd._lib import lib
    from amid_amd.engine import SasrecEngine
    from amid_amd.engine_bert import Bert4recEngine
    switches, build = SCENARIOS[name]
    # (a switch the BERT4Rec engine spells itself is flipped there)
    saved = {(c, k): getattr(c, k) for k in switches for c in (SasrecEngine, Bert4recEngine) if k in vars(c) or (c is SasrecEngine and hasattr(c, k))}
    assert {k for _, k in saved} == set(switches), f"{name}: no engine class has the switch {sorted(set(switches) - {k for _, k in saved})}"
    for (c, k) in saved:
        setattr(c, k, switches[k])
    L = lib()
    try:
        eng, step = build()
        eng.sync()
        L.timer = Tracer(dry)
        step()
        eng.sync()
        return L.timer.lines
    finally:
        L.timer = None
        for (c, k), v in saved.items():
            setattr(c, k, v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenario")
    ap.add_argument("--out")
    ap.add_argument("--dry", action="store_true")
    ap.add_argument("--timeout", type=int, default=90)
    a = ap.parse_args()
    if a.scenario:
        print("\n".join(trace(a.scenario, a.dry)))
        return
    os.makedirs(a.out, exist_ok=True)
    seen, rows = set(), []
    for name in SCENARIOS:
        path = os.path.join(a.out, name + ".trace")
        if a.dry:
            text = "\n".join(trace(name, True)) + "\n"
        else:       # a fresh process under its own time limit; whatever ends it abnormally ends the run
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--scenario", name], capture_output=True, text=True, timeout=a.timeout)
            if r.returncode != 0:
                sys.exit(f"{name}: exit status {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
            text = r.stdout
        open(path, "w").write(text)
        lines = text.splitlines()
        seen |= {ln.split()[0] for ln in lines}
        rows.append((name, len(lines), hashlib.sha256(text.encode()).hexdigest()))
        print(f"{name:32s} {len(lines):3d} {rows[-1][2]}", flush=True)
    must = entries_bound_by_name()
    missing = [e for e in must if not fnmatch.filter(seen, e)]
    assert not missing, f"no scenario launches {missing}"
    print(f"{len(rows)} scenarios, every one of the {len(must)} entry points bound by name appears")


if __name__ == "__main__":
    main()
