"""Score priors for boosted retrieval (VectorIndex.boosted_search, csrc/boosted.hip): host-side math only.

A prior is one float32 per row; a boosted query ranks by cos(q, x_r) + w * prior[r] inside the scan.  `BoostSpec` says
how a prior column is made from what the index knows about its rows -- when they were added and their metadata:

    prior[r] = recency * 2 ** (-max(0, now - t_r) / half_life_s)        (0 where t_r is unknown: NaN)
             + sum over keys of values[key].get(metadata_r.get(key), 0.0)

computed in float64 and rounded to float32 once.  No torch and no GPU in this module.
"""
from __future__ import annotations

import json
import math
import time
from dataclasses import dataclass, field
from typing import Any, Dict, Optional, Sequence

import numpy as np

# bounds of a request's "boost" object (server.py POST /query)
MAX_BOOST_ABS = 10.0
MAX_BOOST_KEYS = 8
MAX_BOOST_VALUES = 32


@dataclass(frozen=True)
class BoostSpec:
    recency: float = 0.0
    half_life_s: float = 30 * 86400.0
    values: Dict[str, Dict[Any, float]] = field(default_factory=dict)
    now: Optional[float] = None     # None: time.time() floored to MMRAG_BOOST_REFRESH_S when the column is built

    def __post_init__(self):
        if not math.isfinite(float(self.recency)):
            raise ValueError("BoostSpec: recency must be finite")
        if not (math.isfinite(float(self.half_life_s)) and float(self.half_life_s) > 0.0):
            raise ValueError("BoostSpec: half_life_s must be a positive number")
        if self.now is not None and not math.isfinite(float(self.now)):
            raise ValueError("BoostSpec: now must be finite")
        for key, table in self.values.items():
            if not isinstance(table, dict):
                raise ValueError(f"BoostSpec: values[{key!r}] must be a dict of value -> weight")
            for w in table.values():
                if not math.isfinite(float(w)):
                    raise ValueError(f"BoostSpec: values[{key!r}] holds a non-finite weight")

    def key(self) -> str:
        """canonical JSON of the spec without `now`: equal specs give equal keys whatever their dicts' order"""
        vals = [[str(k), sorted([[type(v).__name__, str(v), float(w)] for v, w in t.items()])]
                for k, t in sorted(self.values.items(), key=lambda kv: str(kv[0]))]
        return json.dumps({"recency": float(self.recency), "half_life_s": float(self.half_life_s), "values": vals},
                          sort_keys=True, separators=(",", ":"))

    def batch_key(self) -> str:
        """what requests must share to be answered by one boosted search: the spec and its explicit `now`"""
        return f"{self.key()}@{self.now!r}"

    def resolved_now(self, refresh_s: Optional[float] = None, clock=None) -> float:
        """the `now` a column of this spec is built for: the spec's own, else the clock floored to refresh_s"""
        if self.now is not None:
            return float(self.now)
        if refresh_s is None:
            from .config import settings

            refresh_s = float(settings.MMRAG_BOOST_REFRESH_S)
        return floored_now((clock or time.time)(), refresh_s)

    def cache_key(self, refresh_s: Optional[float] = None, clock=None):
        return self.key(), self.resolved_now(refresh_s, clock)

    def column(self, times: np.ndarray, metadatas: Sequence[Dict[str, Any]], now: float) -> np.ndarray:
        """the float32 prior of rows with add times `times` (float64, NaN = unknown) and `metadatas`, at `now`"""
        t = np.asarray(times, dtype=np.float64)
        if t.shape != (len(metadatas),):
            raise ValueError(f"BoostSpec.column: {t.shape[0] if t.ndim else 0} times for {len(metadatas)} rows")
        out = np.zeros(t.shape[0], dtype=np.float64)
        if self.recency != 0.0 and t.size:
            age = np.maximum(0.0, float(now) - np.where(np.isnan(t), float(now), t))
            out += np.where(np.isnan(t), 0.0, float(self.recency) * np.exp2(-age / float(self.half_life_s)))
        for key, table in self.values.items():
            if table and t.size:
                out += np.fromiter((_weight_of(table, m.get(key)) for m in metadatas), dtype=np.float64, count=t.size)
        return out.astype(np.float32)


def _weight_of(table: Dict[Any, float], value) -> float:
    try:
        return float(table.get(value, 0.0))
    except TypeError:        # unhashable metadata value: no table names it
        return 0.0


def floored_now(now: float, refresh_s: float) -> float:
    """`now` floored to a multiple of refresh_s (<= 0: not floored)"""
    refresh_s = float(refresh_s)
    return float(now) if refresh_s <= 0.0 else math.floor(float(now) / refresh_s) * refresh_s


def check_prior_values(values, count: int) -> np.ndarray:
    """a caller's own prior as float32 [count]: finite (after the float32 rounding too), one entry per live row"""
    a = np.asarray(values, dtype=np.float64).reshape(-1)
    if a.shape[0] != count:
        raise ValueError(f"prior holds {a.shape[0]} values for {count} rows")
    with np.errstate(over="ignore"):
        f = a.astype(np.float32)
    if not np.isfinite(f).all():
        raise ValueError("prior values must be finite float32 numbers")
    return f


def parse_boost(raw, default_recency: float = 0.0, default_half_life_days: float = 30.0) -> Optional[BoostSpec]:
    """A request's "boost" field as a BoostSpec, or None when it asks for nothing (absent, false).  `true` takes the
    configured defaults; an object is {"recency": -10..10, "half_life_days": > 0, "values": {key: {value: -10..10}}}
    with at most MAX_BOOST_KEYS keys of MAX_BOOST_VALUES values each.  Raises ValueError with a message fit for a 400."""
    if raw is None or raw is False:
        return None
    if raw is True:
        raw = {}
    if not isinstance(raw, dict):
        raise ValueError("'boost' must be true or an object")
    unknown = set(raw) - {"recency", "half_life_days", "values"}
    if unknown:
        raise ValueError(f"'boost' has unknown fields {sorted(unknown)}")

    def number(name, v, lo, hi, lo_open=False):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(float(v)):
            raise ValueError(f"'boost.{name}' must be a number")
        v = float(v)
        if v > hi or v < lo or (lo_open and v <= lo):
            raise ValueError(f"'boost.{name}' must be in {'(' if lo_open else '['}{lo:g}, {hi:g}]")
        return v

    recency = number("recency", raw.get("recency", default_recency), -MAX_BOOST_ABS, MAX_BOOST_ABS)
    days = number("half_life_days", raw.get("half_life_days", default_half_life_days), 0.0, 36500.0, lo_open=True)
    values = raw.get("values", {})
    if not isinstance(values, dict):
        raise ValueError("'boost.values' must be an object of metadata key -> {value: weight}")
    if len(values) > MAX_BOOST_KEYS:
        raise ValueError(f"'boost.values' names {len(values)} keys, at most {MAX_BOOST_KEYS}")
    tables: Dict[str, Dict[Any, float]] = {}
    for key, table in values.items():
        if not isinstance(key, str) or not key or not isinstance(table, dict):
            raise ValueError("'boost.values' must be an object of metadata key -> {value: weight}")
        if len(table) > MAX_BOOST_VALUES:
            raise ValueError(f"'boost.values.{key}' names {len(table)} values, at most {MAX_BOOST_VALUES}")
        tables[key] = {v: number(f"values.{key}.{v}", w, -MAX_BOOST_ABS, MAX_BOOST_ABS) for v, w in table.items()}
    return BoostSpec(recency=recency, half_life_s=days * 86400.0, values=tables)


def times_to_tables(times: np.ndarray):
    """row add times as the "added_at" list of tables.json: null where unknown"""
    return [None if math.isnan(t) else float(t) for t in np.asarray(times, dtype=np.float64).tolist()]


def times_from_tables(tables: Dict[str, Any], count: int) -> np.ndarray:
    """the row add times of a loaded tables.json: NaN everywhere for a directory written without them"""
    raw = tables.get("added_at")
    if raw is None:
        return np.full(count, np.nan, dtype=np.float64)
    if len(raw) != count:
        raise ValueError(f"tables hold {len(raw)} added_at entries for {count} rows")
    return np.array([np.nan if t is None else float(t) for t in raw], dtype=np.float64)
