"""The Adam tables the launches are bound from (SasrecEngine._adam_dense / _adam_rows) follow the state's buffers: an Adam state that
load_training_state drops and select_optimizer makes again has NEW moments under its old number, and every launch that takes them must be
handed those, not the freed ones."""
import pytest
import torch

from amid_amd import _lib
from amid_amd.engine import SasrecEngine
from oracle import amid_oracle as orc

pytestmark = pytest.mark.gpu
N_ITEMS, D, T, B, NI, HID = 400, 64, 13, 16, 2, 16


def test_a_dropped_and_recreated_adam_state_is_launched_with_its_new_buffers():
    eng = SasrecEngine(N_ITEMS, D, T, HID, lr=1e-3, seed=5)
    eng.load_state_dict(orc.random_params(orc.sasrec_param_shapes(N_ITEMS, D, T, HID, itc_bs=0, inc_bs=0, dr=False), seed=3))
    pl = eng.plan(B, T, NI, need_grad=True)
    b = {k: v.cuda() for k, v in orc.synthetic_batch(B, T, N_ITEMS - 1, pad_id=N_ITEMS - 1, neg=NI - 1, seed=7).items()}
    eng.load_batch(pl, b["i_node"], b["neg_samples"], b["seq_d1"], b["seq_d2"], b["label"], b["domain_id"], None)
    eng.enqueue_train_step(pl)
    state0 = eng.training_state()                       # Adam state 0 alone
    eng.select_optimizer(1)
    eng.enqueue_train_step(pl)                          # state 1: its own moments, used by a step
    eng.sync()
    old = (eng.dense.m, eng.dense.v, eng.table_m, eng.table_v, eng.table_last)      # (kept alive: the new buffers cannot land on their addresses)
    eng.load_training_state(state0)                     # drops state 1
    assert eng.opt_bank == 0 and 1 not in eng._banks
    eng.select_optimizer(1)                             # ... and makes it again
    L, protos, seen = _lib.lib(), _lib.parse_header(), []
    orig = L.call
    L.call = lambda name, *a: (seen.append((name, a)), orig(name, *a))[1]
    try:
        eng.enqueue_train_step(pl)
        eng.sync()
    finally:
        del L.call
    new = (eng.dense.m, eng.dense.v, eng.table_m, eng.table_v, eng.table_last)
    assert all(n is not o and n.data_ptr() != o.data_ptr() for n, o in zip(new, old))
    want = dict(m=new[0], v=new[1], m_tab=new[2], v_tab=new[3], last=new[4])
    checked = 0
    for name, args in seen:
        names = protos[name][2]
        if "m_tab" not in names:
            continue
        for n, t in want.items():
            if n in names and ("p" in names or n not in ("m", "v")):      # (m, v are the dense moments only beside p)
                assert args[names.index(n)] == t.data_ptr(), (name, n)
                checked += 1
    assert checked >= 5                                 # the step's optimizer launch took all five
    assert torch.isfinite(eng.dense.data).all()
