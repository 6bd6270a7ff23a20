"""The launches of one eager step of each driver path, as text: what every C-ABI call was given.  Two trees that print the same traces
hand the same arguments to the same entry points in the same order -- the check of a change to HOW the driver passes arguments
(profiles/launch_trace.md).

One line per launch: the entry name, then every argument.  A scalar is printed by value; a pointer as the ordinal of its first appearance in
the scenario's trace (null = 0), so the line does not depend on where the allocator put things; a host pointer array element by element, a
host int array by its values.  Nothing but lib().timer (the hook bench.py's KernelTimer uses) and the engines' public methods is used, so the
file runs unchanged against another tree's amid_amd/*.py (AMID_TREE) on the same library (AMID_LIB_PATH).

    python profiles/tools/launch_trace.py --out DIR           every scenario, each in a child process under its own time limit (the first
                                                              abnormal exit ends the run), then the coverage check and the table
    python profiles/tools/launch_trace.py --out DIR --dry     ... in this process, recording the calls WITHOUT launching them
    python profiles/tools/launch_trace.py --scenario NAME     one scenario's trace on stdout
"""
import argparse, ctypes, hashlib, os, re, subprocess, sys
ROOT = os.environ.get("AMID_TREE", os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)

# every entry point the driver binds by parameter name must be launched by at least one scenario
MUST_APPEAR = """amid_sas_seq_fwd_f32 amid_sas_seq_fwd_bf16w_f32 amid_sas_seq_fwd_split_f32 amid_sas_seq_fwd_split_lnstat_f32
amid_sas_seq_fwd_split_lnstat_head_f32 amid_sas_seq_fwd_gather_f32 amid_sas_seq_fwd_gather_p1_f32 amid_sas_seq_fwd_gather_head_f32
amid_sas_seq_fwd_gather_head_p1_f32 amid_sas_seq_fwd_gather_infer_f32 amid_sas_seq_fwd_split_infer_f32 amid_sas_seq_bwd_f32
amid_sas_wgrad_rows_sort_ln_f32 amid_sas_strip_qkv_fwd_gather_infer_f32 amid_attn_fwd_long_live_infer_f32
amid_sas_strip_oproj_ffn_fwd_infer_f32 amid_eval_head_f32 amid_eval_head_u_f32 amid_head_fwd_f32 amid_head_bwd_f32
amid_head_fwd_bwd_f32 amid_head_fwd_bwd_own_f32 amid_head_fwd_bwd_own_vec_f32 amid_sas_strip_qkv_bwd_sort_scorer_f32
amid_bert_seq_fwd_gather_infer_f32""".split()

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
})


def trace(name, dry):
    from amid_amd._lib import lib
    from amid_amd.engine import SasrecEngine
    switches, build = SCENARIOS[name]
    saved = {k: getattr(SasrecEngine, k) for k in switches}
    for k, v in switches.items():
        setattr(SasrecEngine, k, v)
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
        for k, v in saved.items():
            setattr(SasrecEngine, k, v)


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
    missing = [e for e in MUST_APPEAR if e not in seen]
    assert not missing, f"no scenario launches {missing}"
    print(f"{len(rows)} scenarios, every one of the {len(MUST_APPEAR)} entry points bound by name appears")


if __name__ == "__main__":
    main()
