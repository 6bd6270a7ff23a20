"""hipGraph capture / replay of the train step and state snapshots (split out of engine.py)."""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from ._lib import lib, ptr_array

from .plan import SasrecPlan


class GraphMixin:
    def capture_local_grads(self, pl: SasrecPlan) -> None:
        L = lib()
        self._ensure_opt_state()
        saved = self.snapshot()
        self.enqueue_local_grads(pl)
        self.sync()
        self.restore(saved)
        self.sync()
        step0 = self.step
        L.call("amid_graph_capture_begin", self.s)
        try:
            self.enqueue_local_grads(pl)
        finally:
            out = ctypes.c_void_p()
            L.call("amid_graph_capture_end", self.s, ctypes.byref(out))
        self.step = step0
        if not isinstance(getattr(pl, "graphs_local", None), dict):
            pl.graphs_local = {}
        pl.graphs_local[self._graph_key()] = out.value      # (keyed like the train-step graphs: the Adam state and the DR objective are baked in)

    def has_local_graph(self, pl: SasrecPlan) -> bool:
        return self._graph_key() in (getattr(pl, "graphs_local", None) or {})


    # ------------------------------------------------------------------ graph replay
    def capture_train_step(self, pl: SasrecPlan) -> None:
        """Capture one train step into a hipGraph (inputs = the plan's static buffers)."""
        L = lib()
        self._ensure_opt_state()
        # warm-up outside capture: sets the dynamic-LDS attributes, pages code objects in
        saved = self.snapshot()
        self.enqueue_train_step(pl)
        self.sync()
        self.restore(saved)
        self.sync()
        s = self.s
        step0 = self.step
        L.call("amid_graph_capture_begin", s)
        try:
            self.enqueue_train_step(pl)
        finally:
            out = ctypes.c_void_p()
            L.call("amid_graph_capture_end", s, ctypes.byref(out))
        self.step = step0          # capture does not execute; the device counter did not move
        if not hasattr(pl, "graphs"):
            pl.graphs = {}
        pl.graphs[self._graph_key()] = out.value       # the Adam state's buffers and the DR objective are baked into a graph
        pl.graph = pl.graphs.get((0, 0), out.value)

    def capture_train_steps(self, pl: SasrecPlan, n_steps: int) -> None:
        """n_steps consecutive train steps as ONE hipGraph (replay_train_steps).  Only with an input pool: every step's first kernel
        picks its batch by the device step counter, so the steps of a graph see consecutive batches; a replayed graph costs ~8 us of
        idle device time between two launches, which a graph of several steps pays once."""
        if self.input_pool(pl) is None:
            raise ValueError("a graph of several train steps needs an input pool (set_input_pool)")
        L = lib()
        if not self.has_graph(pl):
            self.capture_train_step(pl)              # (also the warm-up outside capture)
        s, step0 = self.s, self.step
        L.call("amid_graph_capture_begin", s)
        try:
            for _ in range(n_steps):
                self.enqueue_train_step(pl)
        finally:
            out = ctypes.c_void_p()
            L.call("amid_graph_capture_end", s, ctypes.byref(out))
        self.step = step0
        if not hasattr(pl, "graphs_n"):
            pl.graphs_n = {}
        pl.graphs_n[(self._graph_key(), n_steps)] = out.value

    def replay_train_steps(self, pl: SasrecPlan, n_steps: int) -> None:
        lib().call("amid_graph_launch", pl.graphs_n[(self._graph_key(), n_steps)], self.s)
        self.step += n_steps

    def has_graph(self, pl: SasrecPlan) -> bool:
        return self._graph_key() in getattr(pl, "graphs", {})

    def replay_train_step(self, pl: SasrecPlan) -> None:
        lib().call("amid_graph_launch", pl.graphs[self._graph_key()], self.s)
        self.step += 1

    def flush_table(self) -> None:
        """Apply every pending zero-gradient Adam step (before eval / checkpoint / parity dumps)."""
        if self.table_m is None:
            return
        lib().call("amid_lazy_adam_flush_f32", self.table.data_ptr(), self.table_m.data_ptr(), self.table_v.data_ptr(),
                   self.table_last.data_ptr(), self.n_rows, self.D, self.step_state.data_ptr(), self.s)

    # ------------------------------------------------------------------ snapshots (tests / warm-up)
    def snapshot(self):
        self._ensure_opt_state()
        self.sync()
        fp = self.dense
        # the copies are enqueued on the ENGINE's stream: on torch's they were unordered against the step the caller enqueues next (the
        # warm-up of capture_train_step) -- with a table of a few GB the copy was still running when that step's optimizer moved rows, and
        # restore() put a half-stepped table back (found by test_folded_step_matches_the_fifteen_launch_step at 4.3 M rows, round 6)
        with torch.cuda.stream(self.stream):
            return dict(step=self.step, seed=self.seed, data=fp.data.clone(), m=fp.m.clone(), v=fp.v.clone(), table=self.table.clone(),
                        tm=self.table_m.clone(), tv=self.table_v.clone(), tl=self.table_last.clone())

    def restore(self, snap) -> None:
        fp = self.dense
        with torch.cuda.stream(self.stream):
            fp.data.copy_(snap["data"]); fp.m.copy_(snap["m"]); fp.v.copy_(snap["v"])
            self.table.copy_(snap["table"]); self.table_m.copy_(snap["tm"]); self.table_v.copy_(snap["tv"]); self.table_last.copy_(snap["tl"])
        self.set_step(snap["step"], snap["seed"])

    # ------------------------------------------------------------------ training state (save / resume across processes)
    def _state_config(self) -> Dict[str, object]:
        """The fields a training state must share with the engine that loads it (the buffers' shapes and the step's arithmetic)."""
        return dict(engine=type(self).__name__, n_rows=self.n_rows, D=self.D, T=self.T, Tpos=self.Tpos, hid=self.hid, itc_bs=self.itc_bs,
                    itc_threshold=self.itc_threshold, inc_bs=self.inc_bs, inc_threshold=self.inc_threshold, comp=getattr(self, "comp", ""),
                    dr=self.dr, dr_e_w=self.dr_e_w, compute=self.compute)

    def _bank_buffers(self, k: int) -> dict:
        """Buffers and counters of Adam state `k`: the live one's attributes, or its parked entry (select_optimizer)."""
        if k == self.opt_bank:
            fp = self.dense
            return dict(m=fp.m, v=fp.v, tm=self.table_m, tv=self.table_v, tl=self.table_last, step=self.step, seed=self.seed,
                        lr=self.hyper["lr"])
        return self._banks[k]

    def training_state(self) -> dict:
        """Everything the fused train step carries from one step to the next, as CPU tensors: `config`, `parameters` (the table and
        the flat dense buffer under the reference's state_dict keys) and `optimizer` (per Adam state: dense and table moments,
        table_last, step counter, dropout seed, lr; the live state's number, the DR objective, betas, eps, grad_scale).
        The lazy table state is taken RAW, not flushed: a row with pending zero-gradient steps keeps its table_last, so a resumed run
        replays exactly the steps this one would.  A state that never stepped has no table moments (None); a non-live one that never
        stepped is left out (select_optimizer makes it again as it was).  Derived state -- bf16 weight images, transposes, plans, input
        pools, graphs -- is not saved: it is rebuilt from the parameters every step or batch."""
        self.sync()
        fp = self.dense
        cpu = lambda t: None if t is None else t.to("cpu")      # noqa: E731
        banks = {}
        # (copies on the ENGINE's stream: on torch's they would be unordered against the engine's launches, see snapshot())
        with torch.cuda.stream(self.stream):
            data = fp.data.to("cpu")
            params = {"item_emb_layer.emb_item.weight": self.table.to("cpu")}
            params.update({name: fp.view(name, data).clone() for name in fp.slots})
            for k in sorted(set(self._banks) | {self.opt_bank}):
                b = self._bank_buffers(k)
                if b["tm"] is None and k != self.opt_bank:
                    continue
                banks[int(k)] = dict(m=cpu(b["m"]), v=cpu(b["v"]), table_m=cpu(b["tm"]), table_v=cpu(b["tv"]), table_last=cpu(b["tl"]),
                                     step=int(b["step"]), seed=int(b["seed"]), lr=float(b["lr"]))
        h = self.hyper
        return dict(config=self._state_config(), parameters=params,
                    optimizer=dict(opt_bank=int(self.opt_bank), dr_mode=int(self.dr_mode), betas=(float(h["beta1"]), float(h["beta2"])),
                                   eps=float(h["eps"]), grad_scale=float(self.grad_scale), banks=banks))

    def load_training_state(self, state: dict) -> None:
        """Put a training_state() back, IN PLACE: captured graphs and _ptr_cache hold raw device pointers, so every tensor is copied
        into the buffer the engine already has (on the engine's stream); none is rebound.  The configuration must equal this engine's
        (ValueError naming the first field that differs).  An Adam state the engine lacks is created by select_optimizer, one the state
        lacks is dropped, and then the captured graphs are dropped too (captured again on their next use)."""
        cfg, mine = state.get("config", {}), self._state_config()
        for key, val in mine.items():
            if cfg.get(key) != val:
                raise ValueError(f"training state does not fit this engine: {key} is {cfg.get(key)!r} in the state, {val!r} here")
        params, opt = state["parameters"], state["optimizer"]
        shapes = {"item_emb_layer.emb_item.weight": tuple(self.table.shape), **{n: tuple(s) for n, (_, s) in self.dense.slots.items()}}
        for name, shp in shapes.items():
            if name not in params or tuple(params[name].shape) != shp:
                raise ValueError(f"training state: parameter {name} is missing or not of shape {shp}")
        banks = {int(k): b for k, b in opt["banks"].items()}
        live = int(opt["opt_bank"])
        if live not in banks:
            raise ValueError(f"training state: the live Adam state {live} is missing")
        self.sync()
        have = set(self._banks) | {self.opt_bank}
        for k in sorted(set(banks) - have):
            self.select_optimizer(k)            # (its flush of the state being left is overwritten below)
        self.select_optimizer(live)
        for k in [k for k in self._banks if k not in banks and k != live]:
            del self._banks[k]
        changed = (set(self._banks) | {self.opt_bank}) != have
        for k, s in sorted(banks.items()):
            b = self._bank_buffers(k)
            if s["table_m"] is not None and b["tm"] is None:
                if k == live:
                    self._ensure_opt_state()
                else:
                    b.update(tm=torch.zeros_like(self.table), tv=torch.zeros_like(self.table),
                             tl=torch.zeros(self.n_rows, dtype=torch.int32, device=self.device))
                    torch.cuda.synchronize(self.device)       # (zero-filled on torch's stream, overwritten on the engine's)
                b = self._bank_buffers(k)
            with torch.cuda.stream(self.stream):
                b["m"].copy_(s["m"]); b["v"].copy_(s["v"])
                if s["table_m"] is not None:
                    b["tm"].copy_(s["table_m"]); b["tv"].copy_(s["table_v"]); b["tl"].copy_(s["table_last"])
                elif b["tm"] is not None:       # a state that never stepped: zero moments and stamps are what its first step starts from
                    b["tm"].zero_(); b["tv"].zero_(); b["tl"].zero_()
            if k == live:
                self.step, self.seed, self.hyper["lr"] = int(s["step"]), int(s["seed"]), float(s["lr"])
            else:
                b.update(step=int(s["step"]), seed=int(s["seed"]), lr=float(s["lr"]))
        with torch.cuda.stream(self.stream):
            self.table.copy_(params["item_emb_layer.emb_item.weight"])
            for name in self.dense.slots:
                self.dense.view(name).copy_(params[name])
        self.hyper.update(beta1=float(opt["betas"][0]), beta2=float(opt["betas"][1]), eps=float(opt["eps"]))
        self.dr_mode, self.grad_scale = int(opt["dr_mode"]), float(opt["grad_scale"])
        self._push_step_state()
        if changed:
            self.drop_graphs()
        self.sync()

    def drop_graphs(self) -> None:
        """Forget every captured graph of every plan (train steps, multi-step, evaluation, data parallel): captured again when next used."""
        for pl in self.plans.values():
            for name in ("graphs", "graphs_n", "eval_graphs", "graphs_local", "dp_graphs"):
                g = getattr(pl, name, None)
                if isinstance(g, dict):
                    g.clear()
