"""``Adam``: a drop-in for ``torch.optim.Adam`` in the reference's own training loop, on the engine's dense-equivalent lazy Adam.

    from amid_amd.optim import Adam                       # the one changed import
    optimizer = Adam(model.parameters(), lr=args.lr)      # train_sr.py:480 / train_sr_dr.py:668-669, written as the reference writes it
    for batch in loader:
        predict_d1, predict_d2 = model(...)               # any loss written in torch on the model's outputs
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()

With ``torch.optim.Adam`` that loop materialises the item table's gradient densely in every backward and sweeps the whole table and its two
moment tensors in every step.  With this class the backward leaves the table gradient as the step's segment-reduced unique rows inside the
engine (the table parameter's ``.grad`` stays ``None``), the dense parameters' ``.grad`` are ordinary tensors -- views of one flat buffer --
that autograd accumulates into (the engine's gradient plus whatever else the loss puts on a parameter), and ``step()`` is ONE launch: dense
Adam over the flat buffer and the lazy row Adam over the touched rows (csrc/adam.hip).  The result is the trajectory of
``torch.optim.Adam`` over every parameter, the table included.

No model handle is passed: the optimizer finds the model from the parameters.  It takes the full parameter list of ONE amid_amd model
(``SASRec``, ``BERT4Rec``, ``model_gru.GRU4Rec``, every variant they accept) as one param group, with ``weight_decay = 0``, no ``amsgrad``, no
``maximize``; anything else is a ``ValueError`` that says so.

The contract -- exactly one training-mode forward and backward between two ``step()`` calls:
  * The engine bumps its step counter in every training-mode forward (the lazy catch-up of the rows about to be gathered and the dropout
    counter need it there); Adam's ``t`` counts ``step()`` calls, as torch's does; the rule keeps the two equal.
  * ``step()`` without a backward, after an eval-mode forward only, or after two or more training-mode forwards raises ``RuntimeError`` naming
    the rule; a second ``backward()`` before ``step()`` (gradient accumulation) is refused too: one plan holds one batch's rows.  A refused
    ``step()`` gives the unconsumed bump back: the model trains on.
  * ``zero_grad()`` may come after the forward (the verbatim order): it touches only the ``.grad`` buffer, never what the forward saved.
  * Forwards under ``model.eval()`` BETWEEN steps are free (they flush the lazy rows, as they always did).
  * A table ``.grad`` that is not ``None`` means a loss term touched the table outside the model: refused, never silently densified.

``param_groups[0]["lr"]`` is read at every ``step()``, so ``torch.optim.lr_scheduler.*`` works.  The replay of a row's idle steps takes the
learning rate of the state it runs under, so a CHANGE of lr first brings every row up to date under the old one (one pass over the table):
per-epoch schedules cost nothing to speak of, a per-step schedule pays that pass every step.

Two instances on one model are the reference's ``optimizer`` / ``optimizer2``: instance k drives the engine's Adam state k
(``select_optimizer``), each with its own moments, counter and lr; the first one drives state 0, the state ``model.train_step()`` drives, and
interleaving the two on one model is allowed.  A state is fully flushed when it is left, so the table's values never depend on which state
was active in a forward; only the counters move: the state being left gives back the bump its forward took, the state entered takes it.

``clip_grad_norm_(max_norm)`` is ``torch.nn.utils.clip_grad_norm_`` over every parameter INCLUDING the table's sparse rows (torch's own would
skip the table, whose ``.grad`` is ``None``): the norm is a device scalar, the coefficient stays on the device and the next ``step()`` applies
it inside the optimizer launch -- no host synchronisation.

Data parallel training is not part of this class: the loop has no gradient exchange (use ``model.train_step(exchange=...)``).
"""
from __future__ import annotations

from typing import Optional

import torch

TABLE = "item_emb_layer.emb_item.weight"
RULE = "exactly one training-mode forward and backward between two step() calls"
STATE_FORMAT = 1


def _supported() -> str:
    return ("amid_amd.optim.Adam takes model.parameters() of ONE amid_amd model (SASRec, BERT4Rec, model_gru.GRU4Rec) as one param group, "
            "with weight_decay = 0, amsgrad = False, maximize = False")


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None, maximize=False,
                 capturable=False, differentiable=False, fused=None):
        params = list(params)
        if params and isinstance(params[0], dict):
            if len(params) != 1:
                raise ValueError(f"{len(params)} param groups: " + _supported())
            group = dict(params[0])
            params = list(group.pop("params"))
            lr, betas, eps = group.pop("lr", lr), group.pop("betas", betas), group.pop("eps", eps)
            weight_decay, amsgrad = group.pop("weight_decay", weight_decay), group.pop("amsgrad", amsgrad)
            maximize = group.pop("maximize", maximize)
        if weight_decay != 0 or amsgrad or maximize or differentiable:
            raise ValueError(f"weight_decay = {weight_decay}, amsgrad = {amsgrad}, maximize = {maximize}, differentiable = {differentiable}: "
                             + _supported())
        if isinstance(lr, torch.Tensor) or not lr >= 0.0:
            raise ValueError(f"lr must be a non-negative float, got {lr!r}")
        if not (len(betas) == 2 and 0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0 and eps >= 0.0):
            raise ValueError(f"betas = {betas!r}, eps = {eps!r}: betas in [0, 1) and eps >= 0 are what the engine's step state takes")
        model = self._find_model(params)
        super().__init__(params, dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps), weight_decay=0, amsgrad=False,
                                      maximize=False))
        self._model = model
        eng = model.engine
        self.bank = len(model._amid_optims)          # instance k drives the engine's Adam state k; the first, train_step()'s
        model._amid_optims.append(self)
        self._names = list(model._param_names)
        self._table = model.get_parameter(TABLE)
        self._dense = [(n, model.get_parameter(n)) for n in self._names if n != TABLE]
        if getattr(model, "_amid_gflat", None) is None:
            # the flat buffer the dense parameters' .grad tensors are views of: what autograd accumulates into and the optimizer launch reads
            model._amid_gflat = torch.zeros_like(eng.dense.grad)
            model._amid_gviews = [eng.dense.view(n, model._amid_gflat) for n, _ in self._dense]
            model._amid_dense_params = [p for _, p in self._dense]
            model._amid_sqnorm = torch.zeros(1, dtype=torch.float32, device=eng.device)
        self._clip: Optional[float] = None
        if self.bank == eng.opt_bank:
            eng._ensure_opt_state()                  # from the first forward on, the catch-up runs in front of the gather
            self._sync_hyper(pending=False)

    # ------------------------------------------------------------------ binding
    @staticmethod
    def _find_model(params):
        if not params:
            raise ValueError("an empty parameter list: " + _supported())
        owners = []
        for p in params:
            ref = getattr(p, "_amid_owner", None)
            owner = ref() if ref is not None else None
            if owner is None:
                raise ValueError("a parameter that belongs to no amid_amd model: " + _supported())
            owners.append(owner)
        model = owners[0]
        if any(o is not model for o in owners):
            raise ValueError("parameters of more than one model: " + _supported())
        mine = [id(p) for p in model.parameters()]
        got = [id(p) for p in params]
        if len(set(got)) != len(got) or set(got) != set(mine):
            raise ValueError(f"{len(set(got))} of the model's {len(mine)} parameters: a subset is not supported (the engine's optimizer launch "
                             "steps every parameter).  " + _supported())
        return model

    def add_param_group(self, param_group):
        if getattr(self, "_model", None) is not None or len(self.param_groups) >= 1:
            raise ValueError("a second param group: " + _supported())
        super().add_param_group(param_group)

    # ------------------------------------------------------------------ the engine's Adam state of this instance
    def _hyper(self):
        g = self.param_groups[0]
        lr, (b1, b2), eps = g["lr"], g["betas"], g["eps"]
        if isinstance(lr, torch.Tensor):
            lr = float(lr)
        if g.get("weight_decay", 0) != 0 or g.get("amsgrad", False) or g.get("maximize", False):
            raise ValueError("weight_decay / amsgrad / maximize were switched on in param_groups: " + _supported())
        return dict(lr=float(lr), beta1=float(b1), beta2=float(b2), eps=float(eps))

    def _sync_hyper(self, pending: bool) -> None:
        """Bring the active state's lr / betas / eps to this instance's.  A row's idle steps are replayed with the state's CURRENT values,
        so every row is first brought up to date under the old ones (`pending`: the forward's bump is given back around the flush)."""
        eng = self._model.engine
        want = self._hyper()
        if all(eng.hyper[k] == v for k, v in want.items()):
            return
        if eng.table_m is not None and eng.step - (1 if pending else 0) > 0:
            if pending:
                eng.set_step(eng.step - 1)
            eng.flush_table()
            if pending:
                eng.step += 1
        eng.hyper.update(want)
        eng._push_step_state()

    def _activate(self, pending: bool) -> None:
        """Make this instance's Adam state the engine's live one.  The state being left gives back the bump of a forward it did not get to
        consume (`pending`) and is flushed in full by select_optimizer; the state entered takes the bump."""
        eng = self._model.engine
        if eng.opt_bank != self.bank:
            if pending:
                eng.set_step(eng.step - 1)
            eng.select_optimizer(self.bank)
            if pending:
                eng.set_step(eng.step + 1)
        eng._ensure_opt_state()
        self._sync_hyper(pending)

    # ------------------------------------------------------------------ the loop
    def zero_grad(self, set_to_none: bool = True) -> None:
        """One fill of the flat gradient buffer; every dense parameter's .grad is (again) its view of it, the table's is None.  Nothing
        the forward saved for the backward is touched, so the call may follow the forward."""
        model = self._model
        model._amid_gflat.zero_()
        for (_, p), view in zip(self._dense, model._amid_gviews):
            p.grad = view
        self._table.grad = None

    def _pack(self) -> None:
        """The dense .grad tensors as the flat buffer: nothing to do for the views zero_grad() installed; a .grad autograd or the user
        put in their place (model.zero_grad(), set_to_none) is copied in -- one multi-tensor copy -- and a missing one is zero."""
        model = self._model
        src, dst = [], []
        for (name, p), view in zip(self._dense, model._amid_gviews):
            g = p.grad
            if g is None:
                view.zero_()
            elif g.data_ptr() != view.data_ptr() or g.shape != view.shape or not g.is_contiguous():
                if g.shape != view.shape or g.dtype != view.dtype or g.device != view.device or g.is_sparse:
                    raise ValueError(f"{name}.grad is not a dense float32 tensor of the parameter's shape on its device")
                src.append(g)
                dst.append(view)
        if src:
            torch._foreach_copy_(dst, src)

    def _abandon(self) -> None:
        """A refused step: the forward's bump, if there was one, goes back; the counters start over."""
        model = self._model
        if model._loop["fwd"]:
            model.engine.set_step(model.engine.step - 1)
        model._loop["fwd"] = model._loop["bwd"] = 0
        for o in model._amid_optims:
            o._clip = None

    def _check_loop(self, what: str) -> None:
        loop = self._model._loop
        if loop["bwd"] == 0:
            fwd = loop["fwd"]
            self._abandon()
            raise RuntimeError(f"{what} without a backward() ({fwd} training-mode forward(s) since the last step()): {RULE}")
        if loop["fwd"] != 1:
            fwd = loop["fwd"]
            self._abandon()
            raise RuntimeError(f"{what} after {fwd} training-mode forwards (model.train()) since the last step(): {RULE}")
        if self._table.grad is not None:
            self._table.grad = None
            self._abandon()
            raise ValueError("the item table's .grad is set: a loss term touched item_emb_layer.emb_item.weight outside the model.  The table "
                             "gradient stays the step's sparse rows here and is not densified; put such a term through the model's outputs, or "
                             "use torch.optim.Adam")

    @torch.no_grad()
    def clip_grad_norm_(self, max_norm, norm_type: float = 2.0, error_if_nonfinite: bool = False, foreach=None) -> torch.Tensor:
        """torch.nn.utils.clip_grad_norm_ over every parameter, the table's sparse rows included; call it between backward() and step().
        Returns the total norm as a 0-dim device tensor; the clip itself happens inside the next step()'s launch."""
        if float(norm_type) != 2.0:
            raise ValueError(f"norm_type {norm_type!r}: only the 2-norm is built")
        if error_if_nonfinite:
            raise ValueError("error_if_nonfinite needs the norm on the host: not supported (the norm never leaves the device)")
        max_norm = float(max_norm)
        if not max_norm >= 0.0:
            raise ValueError(f"max_norm must be >= 0, got {max_norm!r}")
        self._check_loop("clip_grad_norm_()")
        model = self._model
        eng, pl = model.engine, model._last_plan
        self._pack()
        eng.stream.wait_stream(torch.cuda.current_stream())
        eng.enqueue_grad_sqnorm(pl, model._amid_gflat, model._amid_sqnorm)
        torch.cuda.current_stream().wait_stream(eng.stream)
        self._clip = max_norm
        return model._amid_sqnorm[0].sqrt()

    @torch.no_grad()
    def step(self, closure=None):
        if closure is not None:
            raise ValueError("a closure would run a second forward and backward: " + RULE)
        self._check_loop("step()")
        model = self._model
        eng, pl = model.engine, model._last_plan
        self._pack()
        try:
            self._activate(pending=True)
        except Exception:
            self._abandon()
            raise
        eng.stream.wait_stream(torch.cuda.current_stream())
        if self._clip is not None:
            eng.enqueue_loop_optimizer(pl, model._amid_gflat, model._amid_sqnorm, self._clip)
        else:
            eng.enqueue_loop_optimizer(pl, model._amid_gflat)
        torch.cuda.current_stream().wait_stream(eng.stream)
        model._loop["fwd"] = model._loop["bwd"] = 0
        for o in model._amid_optims:
            o._clip = None
        return None

    # ------------------------------------------------------------------ state
    def state_dict(self) -> dict:
        """This instance's Adam state -- dense and table moments, the per-row stamps, the step counter, the dropout seed, lr: what
        SasrecEngine.training_state() saves for one state -- as CPU tensors and plain data (torch.save / torch.load(weights_only=True)).
        The lazy rows are brought up to date first, as model.state_dict() does, so the two may be taken in either order."""
        model = self._model
        eng = model.engine
        if model._loop["fwd"] or model._loop["bwd"]:
            raise RuntimeError("state_dict() between a forward and its step(): " + RULE)
        self._activate(pending=False)
        eng.flush_table()
        eng.sync()
        fp = eng.dense
        cpu = lambda t: t.detach().to("cpu").clone()      # noqa: E731
        with torch.cuda.stream(eng.stream):
            state = dict(step=int(eng.step), seed=int(eng.seed), lr=float(eng.hyper["lr"]), m=cpu(fp.m), v=cpu(fp.v), table_m=cpu(eng.table_m),
                         table_v=cpu(eng.table_v), table_last=cpu(eng.table_last))
        eng.sync()
        g = self.param_groups[0]
        group = {k: (list(v) if isinstance(v, tuple) else v) for k, v in g.items() if k != "params" and isinstance(v, (int, float, bool, tuple, list, type(None)))}
        group["params"] = list(range(len(g["params"])))
        return {"format": STATE_FORMAT, "bank": int(self.bank), "state": state, "param_groups": [group]}

    def load_state_dict(self, state_dict: dict) -> None:
        """Put a state_dict() back, in place (captured graphs hold the buffers' addresses): a fresh model + optimizer loaded with both
        state dicts continues bit for bit."""
        model = self._model
        eng = model.engine
        if state_dict.get("format") != STATE_FORMAT or "state" not in state_dict:
            raise ValueError(f"not an amid_amd.optim.Adam state of format {STATE_FORMAT}")
        if model._loop["fwd"] or model._loop["bwd"]:
            raise RuntimeError("load_state_dict() between a forward and its step(): " + RULE)
        s, fp = state_dict["state"], eng.dense
        if tuple(s["m"].shape) != tuple(fp.m.shape) or tuple(s["table_m"].shape) != tuple(eng.table.shape):
            raise ValueError("the state's moments do not have this model's shapes")
        group = state_dict["param_groups"][0]
        mine = self.param_groups[0]
        for k, v in group.items():
            if k != "params":
                mine[k] = tuple(v) if k == "betas" else v
        mine["lr"] = float(s["lr"])
        self._activate(pending=False)
        eng.sync()
        with torch.cuda.stream(eng.stream):
            fp.m.copy_(s["m"]); fp.v.copy_(s["v"])
            eng.table_m.copy_(s["table_m"]); eng.table_v.copy_(s["table_v"]); eng.table_last.copy_(s["table_last"])
        eng.hyper.update(self._hyper())
        eng.set_step(int(s["step"]), int(s["seed"]))
        eng.sync()
