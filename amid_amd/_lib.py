"""ctypes binding of ``libamid_hip.so`` (the C ABI declared in ``include/amid_hip.h``).

The prototypes are parsed from the header itself, so the binding cannot drift
from the declared ABI, and :func:`declared_symbols` is what the CPU-side test
uses to check that the built library exports every declared entry point.

There is no fallback: if the shared library is missing or a symbol cannot be
resolved, importing the compute path raises (``AmidLibraryError``).
"""
from __future__ import annotations

import ctypes
import operator
import os
import re
from typing import Dict, List, Tuple

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AMID_LIB_PATH") or os.path.join(_HERE, "libamid_hip.so")      # (AMID_LIB_PATH: diagnostic builds)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "amid_hip.h")


class AmidLibraryError(RuntimeError):
    pass


class AmidError(RuntimeError):
    def __init__(self, fn: str, code: int, text: str):
        super().__init__(f"{fn} failed with code {code}: {text}")
        self.fn, self.code = fn, code


_SCALARS = {
    "int": ctypes.c_int,
    "float": ctypes.c_float,
    "double": ctypes.c_double,
    "long long": ctypes.c_longlong,
    "unsigned long long": ctypes.c_ulonglong,
    "unsigned": ctypes.c_uint,
    "unsigned int": ctypes.c_uint,
}


def _ctype_of(decl: str):
    """C parameter/return declaration (without the name) -> ctypes type."""
    d = decl.replace("const", " ").strip()
    d = re.sub(r"\s+", " ", d)
    if d == "char*":
        return ctypes.c_char_p
    if "*" in d:
        return ctypes.c_void_p
    if d == "void":
        return None
    return _SCALARS[d]


def parse_prototypes(text: str) -> Dict[str, Tuple[object, List[object], List[str]]]:
    """Entry point -> (ctypes return type, ctypes parameter types, parameter names) for every ``amid_*`` prototype in `text`."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)      # drop comments
    text = re.sub(r"//[^\n]*", " ", text)
    protos: Dict[str, Tuple[object, List[object], List[str]]] = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(amid_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        argtypes, names = [], []
        if args and args != "void":
            for a in args.split(","):
                a = a.strip()
                mm = re.match(r"^(.*?)([A-Za-z_]\w*)$", a, flags=re.S)   # the declaration, the parameter name
                argtypes.append(_ctype_of(mm.group(1)))
                names.append(mm.group(2))
        protos[name] = (_ctype_of(ret), argtypes, names)
    return protos


def parse_header(path: str = HEADER_PATH) -> Dict[str, Tuple[object, List[object], List[str]]]:
    return parse_prototypes(open(path).read())


class Binder:
    """Named arguments -> the positional order of a prototype.  The values come from `tables` (mappings parameter name -> value: the
    engines' named pointer tables; names the entry point does not take are ignored, which is how one table serves entry points that
    take a subset of it) and from `args` (every name must be a parameter).  Every parameter must be supplied exactly once -- null is
    an explicit None --, otherwise TypeError naming the entry point and the parameter: nothing is launched.  That is checked once per
    (entry point, names supplied by each source); after that a bind merges the sources and picks the parameters in order."""

    def __init__(self, protos) -> None:
        self._params = {entry: tuple(p[2]) for entry, p in protos.items()}
        self._orders: Dict[tuple, list] = {}

    def bind(self, entry: str, tables, args) -> tuple:
        key = (entry, tuple(map(tuple, tables)), tuple(args))
        pick = self._orders.get(key)
        if pick is None:
            pick = self._orders[key] = self._resolve(entry, tables, args)
        merged = {}
        for t in tables:
            merged.update(t)
        merged.update(args)
        return pick(merged)

    def _resolve(self, entry: str, tables, args):
        """The check of one (entry point, names supplied by each source): every parameter from exactly one source.  Returns what picks the
        parameters, in the prototype's order, out of the sources merged into one mapping (no name is in two of them: checked here)."""
        params = self._params.get(entry)
        if params is None:
            raise TypeError(f"{entry} is not declared in include/amid_hip.h")
        for n in args:
            if n not in params:
                raise TypeError(f"{entry} has no parameter {n!r}")
        for n in params:
            at = [i for i, src in enumerate((*tables, args)) if n in src]
            if len(at) != 1:
                raise TypeError(f"{entry}: parameter {n!r} " + ("is not supplied (null is an explicit None)" if not at else
                                                               f"is supplied {len(at)} times"))
        if len(params) < 2:          # (itemgetter gives a bare value for one name and takes no empty list)
            return lambda merged: tuple(merged[n] for n in params)
        return operator.itemgetter(*params)


def prefixed(prefix: str, table) -> dict:
    """`table` under the names an entry point spells with `prefix`: the fused feed-forward chain of the q / k / v backward (fh, fr, fln_w ...),
    the next layer's q / k / v of an out-projection / feed-forward forward (nln_w, nqn ...)."""
    return {prefix + k: v for k, v in table.items()}


def absent(table, **scalars) -> dict:
    """An optional block an entry point is not given: every name of `table` as an explicit null (`scalars`: the block's by-value parameters)."""
    return {**dict.fromkeys(table), **scalars}


def declared_symbols() -> List[str]:
    return sorted(parse_header())


class _Lib:
    def __init__(self) -> None:
        if not os.path.exists(LIB_PATH):
            raise AmidLibraryError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                f"(or `make -C amid_amd/csrc`).  There is no CPU fallback for the amid_amd compute path.")
        try:
            self._dll = ctypes.CDLL(LIB_PATH)
        except OSError as e:  # pragma: no cover
            raise AmidLibraryError(f"cannot load {LIB_PATH}: {e}") from e
        self._fn = {}
        self.timer = None          # optional KernelTimer (bench.py): HIP events around every launch
        protos = parse_header()
        self._binder = Binder(protos)
        for name, (restype, argtypes, _) in protos.items():
            try:
                f = getattr(self._dll, name)
            except AttributeError as e:
                raise AmidLibraryError(f"{LIB_PATH} does not export {name} declared in include/amid_hip.h") from e
            f.restype = restype
            f.argtypes = argtypes
            self._fn[name] = f

    def raw(self, name: str):
        return self._fn[name]

    def call(self, name: str, *args) -> None:
        """Call an int-returning entry point; raise AmidError on a non-zero code."""
        if self.timer is not None and name not in _UNTIMED:
            return self.timer.timed_call(self, name, args)
        code = self._fn[name](*args)
        if code != 0:
            text = self._fn["amid_error_string"](code)
            raise AmidError(name, code, text.decode() if text else "?")

    def call_named(self, name: str, *tables, **args) -> None:
        """call() with the arguments given by parameter name (Binder): the wide launches' form.  The header's parameter names are
        part of what this relies on."""
        return self.call(name, *self._binder.bind(name, tables, args))

    def value(self, name: str, *args):
        """Call an entry point that returns a plain value (sizes, counts)."""
        return self._fn[name](*args)


_UNTIMED = {"amid_event_create", "amid_event_record", "amid_event_sync", "amid_event_elapsed_ms", "amid_event_destroy",
            "amid_graph_capture_begin", "amid_graph_capture_end", "amid_graph_launch", "amid_graph_destroy", "amid_step_state_pack",
            "amid_reduce_entry_pack"}


class KernelTimer:
    """Brackets every kernel-launching C-ABI call with HIP events recorded on the stream the kernels
    run on (the last argument of every launching entry point); durations are read after a sync."""

    def __init__(self, only=None):
        self.records = []      # (name, start_event, stop_event)
        self.only = only       # optional set of entry names: the others are launched without events (a queue that stays full)

    def timed_call(self, L: "_Lib", name: str, args) -> None:
        if self.only is not None and name not in self.only:
            code = L._fn[name](*args)
            if code != 0:
                text = L._fn["amid_error_string"](code)
                raise AmidError(name, code, text.decode() if text else "?")
            return
        stream = args[-1]
        e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
        L._fn["amid_event_create"](ctypes.byref(e0))
        L._fn["amid_event_create"](ctypes.byref(e1))
        L._fn["amid_event_record"](e0, stream)
        code = L._fn[name](*args)
        L._fn["amid_event_record"](e1, stream)
        self.records.append((name, e0, e1))
        if code != 0:
            text = L._fn["amid_error_string"](code)
            raise AmidError(name, code, text.decode() if text else "?")

    def collect(self, L: "_Lib") -> Dict[str, List[float]]:
        """name -> list of durations in ms (call order preserved); destroys the events."""
        out: Dict[str, List[float]] = {}
        for name, e0, e1 in self.records:
            L._fn["amid_event_sync"](e1)
            ms = ctypes.c_float()
            L._fn["amid_event_elapsed_ms"](e0, e1, ctypes.byref(ms))
            out.setdefault(name, []).append(float(ms.value))
            L._fn["amid_event_destroy"](e0)
            L._fn["amid_event_destroy"](e1)
        self.records = []
        return out


_LIB = None


def lib() -> _Lib:
    global _LIB
    if _LIB is None:
        _LIB = _Lib()
    return _LIB


def ptr_array(ptrs) -> ctypes.Array:
    """Host array of device pointers for the ``const float* const*`` parameters."""
    arr = (ctypes.c_void_p * len(ptrs))()
    for i, p in enumerate(ptrs):
        arr[i] = p
    return arr
