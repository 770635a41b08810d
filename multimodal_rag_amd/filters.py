"""Metadata filters on the device: the compiler from a `where` dict to a small postfix program, a numpy interpreter of
that program, and the typed metadata columns a VectorIndex keeps for it (include/mmrag.h mmrag_filter_eval,
csrc/filtered.hip).  Pure Python + numpy up to ColumnRegistry.device(), which uploads.

The semantic reference is index.match_where.  What is covered compiles to a program whose result equals match_where on
every row; anything else is refused with a reason and takes the host path.

Columns, one per metadata key, built on first use of the key in a device filter:
    NUMBER   float64, NaN = the key is missing or None; values: bool, int with |v| <= 2**53, finite float
    STRING   int32 ordinals into a per-key dictionary in first-seen order, -1 = missing or None; values: str only
Any other value (a float NaN, a larger int, a list, a str among numbers) makes the key UNSUPPORTED from then on.  A key
no row has is ABSENT: every leaf on it is the constant match_where gives for None.  The reserved key "$added_at" is the
NUMBER column of the rows' add times.

A row's operand is its column value as a double (an ordinal of -1 as NaN).  IEEE comparisons against NaN give
match_where's answers for a missing value -- false for == > >= < <= in, true for != not-in -- so a program has no case
for it.
"""
from __future__ import annotations

import math
from typing import Any, Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

# instruction codes and column kinds of include/mmrag.h
TRUE, FALSE, AND, OR, EQ, NE, GT, GE, LT, LE, IN, NIN = range(12)
NUMBER, STRING = 0, 1
ABSENT, UNSUPPORTED = -1, -2
MAX_FILTER_OPS = 32
MAX_FILTER_SET = 64
MAX_FILTER_COLUMNS = 16
ADDED_AT = "$added_at"
MAX_EXACT_INT = 2 ** 53

_OPS = {"$eq": EQ, "$ne": NE, "$gt": GT, "$gte": GE, "$lt": LT, "$lte": LE, "$in": IN, "$nin": NIN}
_ON_NONE = {EQ: False, NE: True, GT: False, GE: False, LT: False, LE: False, IN: False, NIN: True}

# the layout of mmrag_filter_op (24 bytes)
OP_DTYPE = np.dtype([("code", "<i4"), ("column", "<i4"), ("set_off", "<i4"), ("set_len", "<i4"), ("value", "<f8")])


class Instr(NamedTuple):
    code: int
    key: Optional[str] = None      # the column of a comparison
    value: float = 0.0             # EQ .. LE
    values: Tuple[float, ...] = () # IN / NIN: ascending


class Program(NamedTuple):
    """a compiled filter: postfix instructions; equal filters give equal (and equally hashing) programs"""
    instrs: Tuple[Instr, ...]

    @property
    def keys(self) -> List[str]:
        """the columns it reads, in order of first use"""
        out: List[str] = []
        for ins in self.instrs:
            if ins.key is not None and ins.key not in out:
                out.append(ins.key)
        return out


class Refused(Exception):
    """the filter is not covered by the device path; str(e) is the reason"""


def is_number(v: Any) -> bool:
    """a value a NUMBER column or constant may hold"""
    if isinstance(v, bool):
        return True
    if isinstance(v, int):
        return abs(v) <= MAX_EXACT_INT
    return isinstance(v, float) and math.isfinite(v)


def _constant(key: str, col, v: Any) -> Optional[float]:
    """constant v of a leaf on `col` as the double the program compares with; None = equal to no stored value"""
    if v is None:
        raise Refused(f"a None constant on {key!r}")
    if col is None or col.kind == ABSENT:
        if not (is_number(v) or isinstance(v, str)):
            raise Refused(f"the constant {v!r} on {key!r} is neither a number nor a string")
        return None
    if col.kind == NUMBER:
        if not is_number(v):
            raise Refused(f"{key!r} is a number column; the constant {v!r} is not a number it can hold")
        return float(v)
    if not isinstance(v, str):
        raise Refused(f"{key!r} is a string column; the constant {v!r} is not a string")
    o = col.ordinals.get(v)
    return None if o is None else float(o)


def _leaf(kinds, key: str, code: int, val: Any) -> Instr:
    col = kinds.get(key)
    if col is not None and col.kind == UNSUPPORTED:
        raise Refused(f"key {key!r} is unsupported: {col.reason}")
    const = lambda b: Instr(TRUE if b else FALSE)                              # noqa: E731
    if code in (IN, NIN):
        if not isinstance(val, (list, tuple, set, frozenset)):
            raise Refused(f"the operand of $in / $nin on {key!r} is not a list")
        if not 1 <= len(val) <= MAX_FILTER_SET:
            raise Refused(f"a $in / $nin list of {len(val)} values on {key!r} (1..{MAX_FILTER_SET})")
        got = sorted({c for c in (_constant(key, col, v) for v in val) if c is not None})
        if not got:
            return const(code == NIN)
        return Instr(code, key, 0.0, tuple(got))
    if col is not None and col.kind == STRING and code not in (EQ, NE):
        raise Refused(f"an ordering operator on the string column {key!r}")
    c = _constant(key, col, val)
    if c is None:
        return const(_ON_NONE[code]) if col is None or col.kind == ABSENT else const(code == NE)
    return Instr(code, key, c)


def _joined(parts: List[List[Instr]], code: int) -> List[Instr]:
    """postfix of parts[0] CODE parts[1] CODE ...; no part: the neutral element"""
    if not parts:
        return [Instr(TRUE if code == AND else FALSE)]
    out = list(parts[0])
    for p in parts[1:]:
        out += p
        out.append(Instr(code))
    return out


def _compile(where, kinds) -> List[Instr]:
    if not where:
        return [Instr(TRUE)]
    if not isinstance(where, dict):
        raise Refused(f"a filter must be a dict, not {type(where).__name__}")
    parts: List[List[Instr]] = []
    for key in sorted(where, key=repr):          # canonical: equal dicts compile to one program
        cond = where[key]
        if key in ("$and", "$or"):
            if not isinstance(cond, (list, tuple)):
                raise Refused(f"{key} takes a list of filters")
            parts.append(_joined([_compile(w, kinds) for w in cond], AND if key == "$and" else OR))
        elif isinstance(cond, dict):
            for op in cond:
                if op not in _OPS:
                    raise ValueError(f"unsupported where operator {op!r}")        # match_where's own error
            if not isinstance(key, str):
                raise Refused(f"the key {key!r} is not a string")
            for op in sorted(cond):
                parts.append([_leaf(kinds, key, _OPS[op], cond[op])])
        else:
            if not isinstance(key, str):
                raise Refused(f"the key {key!r} is not a string")
            if isinstance(cond, (list, tuple, set, frozenset)):
                raise Refused(f"equality with a list on {key!r}")
            parts.append([_leaf(kinds, key, EQ, cond)])
    return _joined(parts, AND)


def try_compile(where, kinds) -> Tuple[Optional[Program], str]:
    """(program, "") or (None, why the device path does not cover `where`).  `kinds` maps a metadata key to its column
    (an object with .kind and, for strings, .ordinals), None for a key no row has: a ColumnRegistry, or a dict.  An
    unknown operator raises ValueError as match_where does."""
    try:
        instrs = _compile(where, kinds)
    except Refused as e:
        return None, str(e)
    if len(instrs) > MAX_FILTER_OPS:
        return None, f"a program of {len(instrs)} instructions (at most {MAX_FILTER_OPS})"
    prog = Program(tuple(instrs))
    if len(prog.keys) > MAX_FILTER_COLUMNS:
        return None, f"a filter over {len(prog.keys)} keys (at most {MAX_FILTER_COLUMNS})"
    return prog, ""


def compile_where(where, kinds) -> Optional[Program]:
    """the program of `where`, or None when the device path does not cover it (try_compile gives the reason)"""
    return try_compile(where, kinds)[0]


def names_added_at(where) -> bool:
    """whether the filter names the reserved key "$added_at" anywhere"""
    if isinstance(where, dict):
        return any(k == ADDED_AT or (k in ("$and", "$or") and names_added_at(v)) for k, v in where.items())
    if isinstance(where, (list, tuple)):
        return any(names_added_at(w) for w in where)
    return False


def _operand(col: np.ndarray) -> np.ndarray:
    """a column's values as the doubles a program compares: ordinals below 0 as NaN"""
    a = np.asarray(col)
    if a.dtype.kind in "iu":
        out = a.astype(np.float64)
        out[a < 0] = np.nan
        return out
    return a.astype(np.float64, copy=False)


def run_program_host(program: Program, columns: Dict[str, np.ndarray], n: Optional[int] = None) -> np.ndarray:
    """bool[n]: the program on every row, in numpy -- the same instructions with the same IEEE comparisons as
    filter_eval_kernel.  `columns`: key -> float64 values (NUMBER) or int32 ordinals (STRING), each of n rows or more;
    `n` defaults to the shortest column given."""
    if n is None:
        n = min((len(c) for c in columns.values()), default=0)
    stack: List[np.ndarray] = []
    with np.errstate(invalid="ignore"):
        for ins in program.instrs:
            if ins.code in (TRUE, FALSE):
                stack.append(np.full(n, ins.code == TRUE, dtype=bool))
            elif ins.code in (AND, OR):
                b, a = stack.pop(), stack.pop()
                stack.append(a & b if ins.code == AND else a | b)
            else:
                v = _operand(columns[ins.key][:n])
                if ins.code in (IN, NIN):
                    hit = np.isin(v, np.asarray(ins.values, dtype=np.float64))
                    stack.append(hit if ins.code == IN else ~hit)
                else:
                    x = ins.value
                    stack.append({EQ: v == x, NE: v != x, GT: v > x, GE: v >= x, LT: v < x, LE: v <= x}[ins.code])
    return stack[-1]


def pack_bits(flags: np.ndarray, words: int) -> np.ndarray:
    """bool[n] as `words` uint32 words, bit r & 31 of word r >> 5 = row r"""
    out = np.zeros(words * 32, dtype=bool)
    out[: flags.size] = flags
    return np.packbits(out, bitorder="little").view(np.uint32)


def pack_programs(programs: Sequence[Program]):
    """The device tables of mmrag_filter_eval for these programs: (ops [n_ops] OP_DTYPE, prog_off [F + 1] int32,
    set_values [n_set] float64, keys) -- `keys` is the launch's column list, an instruction's `column` indexes it."""
    keys: List[str] = []
    ops, off, sets = [], [0], []
    for prog in programs:
        for ins in prog.instrs:
            column = 0
            if ins.key is not None:
                if ins.key not in keys:
                    keys.append(ins.key)
                column = keys.index(ins.key)
            ops.append((ins.code, column, len(sets) if ins.values else 0, len(ins.values), ins.value))
            sets.extend(ins.values)
        off.append(len(ops))
    return (np.array(ops, dtype=OP_DTYPE), np.array(off, dtype=np.int32), np.array(sets, dtype=np.float64), keys)


# --------------------------------------------------------------------------------------------
# the columns
# --------------------------------------------------------------------------------------------
class Column:
    """one metadata key's typed column: kind, dictionary (strings), host mirror and, once asked for, device tensor"""

    def __init__(self, key: str):
        self.key = key
        self.kind = ABSENT
        self.reason = ""
        self.ordinals: Dict[str, int] = {}     # STRING: value -> ordinal, first-seen order
        self.host: Optional[np.ndarray] = None  # float64 / int32, at least the rows in use
        self.dev = None                         # torch tensor [capacity], rows [0, synced) current
        self.synced = 0

    def _drop(self, reason: str):
        self.kind, self.reason = UNSUPPORTED, reason
        self.ordinals, self.host, self.dev, self.synced = {}, None, None, 0

    def _room(self, n: int):
        fill = np.nan if self.kind == NUMBER else -1
        if self.host is None or self.host.size < n:
            new = np.full(max(n, 2 * (self.host.size if self.host is not None else 0), 256), fill,
                          dtype=np.float64 if self.kind == NUMBER else np.int32)
            if self.host is not None:
                new[: self.host.size] = self.host
            self.host = new

    def extend(self, values: List[Any], lo: int):
        """rows lo .. lo + len(values) hold these values of the key (None = missing); one batch, no per-row numpy"""
        if self.kind == UNSUPPORTED:
            return
        present = [v for v in values if v is not None]
        if not present:
            if self.kind != ABSENT:
                self._room(lo + len(values))      # the fill is "missing"
            return
        types = set(map(type, present))
        if self.kind == ABSENT:
            self.kind = STRING if types == {str} else NUMBER
        hi = lo + len(values)
        if self.kind == NUMBER:
            if not types <= {bool, int, float}:
                return self._drop("a value that is not a number: " + ", ".join(sorted(t.__name__ for t in types)))
            if int in types and max(abs(v) for v in present if type(v) is int) > MAX_EXACT_INT:
                return self._drop("an int beyond 2**53")
            arr = np.array([np.nan if v is None else v for v in values], dtype=np.float64)
            if float in types and (int(np.isnan(arr).sum()) != len(values) - len(present) or np.isinf(arr).any()):
                return self._drop("a float that is not finite")
            self._room(hi)
            self.host[lo:hi] = arr
        else:
            if types != {str}:
                return self._drop("a value that is not a string: " + ", ".join(sorted(t.__name__ for t in types)))
            ordinals = self.ordinals
            for v in present:
                if v not in ordinals:
                    ordinals[v] = len(ordinals)
            self._room(hi)
            self.host[lo:hi] = [-1 if v is None else ordinals[v] for v in values]


class _TimesColumn:
    """the reserved "$added_at": the owner's add times, NaN where unknown; the host mirror is the owner's own array"""
    key, kind, reason, ordinals = ADDED_AT, NUMBER, "", {}

    def __init__(self):
        self.dev = None
        self.synced = 0


class ColumnRegistry:
    """The typed metadata columns of one collection.  `rows()` -> (metadatas, n, add_times or None) is the owner's view
    of its row tables; the owner calls appended / compacted / reset as they change (VectorIndex, under its lock).  A
    column is built on the first get(key): one pass over the n metadatas."""

    def __init__(self, rows: Callable[[], Tuple[Sequence[Dict[str, Any]], int, Optional[np.ndarray]]]):
        self._rows = rows
        self._cols: Dict[str, Column] = {}
        self._times = _TimesColumn()

    @classmethod
    def from_metadatas(cls, metadatas: Sequence[Dict[str, Any]], times: Optional[np.ndarray] = None) -> "ColumnRegistry":
        metas = list(metadatas)
        return cls(lambda: (metas, len(metas), times))

    def get(self, key: str):
        """the key's column (built now if this is its first use); None never: an unknown key is an ABSENT column"""
        if key == ADDED_AT:
            return self._times
        col = self._cols.get(key)
        if col is None:
            metas, n, _ = self._rows()
            col = self._cols[key] = Column(key)
            col.extend([m.get(key) for m in metas[:n]], 0)
        return col

    def host(self, key: str) -> np.ndarray:
        """the host mirror of a NUMBER / STRING column: at least n values"""
        if key == ADDED_AT:
            _, n, times = self._rows()
            return times if times is not None else np.full(n, np.nan)
        return self.get(key).host

    def host_columns(self, keys: Sequence[str]) -> Dict[str, np.ndarray]:
        n = self._rows()[1]
        return {k: self.host(k)[:n] for k in keys}

    def appended(self, metadatas: Sequence[Dict[str, Any]], lo: int):
        """rows lo .. lo + len(metadatas) were appended with these metadatas"""
        for col in self._cols.values():
            key = col.key
            col.extend([m.get(key) for m in metadatas], lo)

    def compacted(self, keep: np.ndarray):
        """the rows `keep` (ascending) are now rows 0 .. len(keep); dictionaries keep their ordinals"""
        for col in self._cols.values():
            if col.host is not None:
                col.host = col.host[keep]
            col.synced = 0
        self._times.synced = 0

    def reset(self):
        self._cols = {}
        self._times = _TimesColumn()

    def device(self, key: str, capacity: int, device):
        """the column as a device tensor [capacity] with rows 0 .. n current (float64 or int32): rows appended since the
        last call are uploaded, everything after a growth or a compaction"""
        import torch

        col = self.get(key)
        n = self._rows()[1]
        host = self.host(key)
        dtype = torch.float64 if col.kind == NUMBER else torch.int32
        if col.dev is None or col.dev.numel() < max(capacity, n, 1) or col.dev.device != torch.device(device):
            col.dev = torch.empty(max(capacity, n, 1), dtype=dtype, device=device)
            col.synced = 0
        if col.synced < n:
            col.dev[col.synced:n].copy_(torch.from_numpy(np.ascontiguousarray(host[col.synced:n])))
        col.synced = n
        return col.dev

    def plan(self, where) -> Dict[str, Any]:
        """{"device": bool, "reason": str, "columns": [keys]} for `where`"""
        prog, why = try_compile(where, self)
        return {"device": prog is not None, "reason": why, "columns": prog.keys if prog is not None else []}
