"""The points of a parameter scan, for the engines that have one (ensemble.py, mdlc.py) and their tools."""
from __future__ import annotations

import ctypes as C
import itertools


def sweep_points(base, sweep, fields):
    """(the points' swept values as dicts, the points as a C array of type(base)): the Cartesian product of the
    lists of `sweep` ({name: values}), the first-named axis slowest — or, where `sweep` is a list of {name: value}
    dicts, those points as they stand; the names from `fields`, every other field from `base`"""
    if isinstance(sweep, dict):
        names = list(sweep)
        for name in names:
            if len(sweep[name]) < 1:
                raise ValueError(f"sweep: no values for {name!r}")
        values = [dict(zip(names, v)) for v in itertools.product(*(sweep[n] for n in names))]
    else:
        values = [dict(point) for point in sweep]
        if not values:
            raise ValueError("sweep: no points")
    for name in {n for point in values for n in point}:
        if name not in fields:
            raise ValueError(f"sweep: {name!r} is not one of {', '.join(fields)}")
    params = type(base)
    arr = (params * len(values))()
    for q, point in enumerate(values):
        C.memmove(C.byref(arr[q]), C.byref(base), C.sizeof(params))
        for name, v in point.items():
            setattr(arr[q], name, float(v))
    return values, arr


def parse_sweep_args(items):
    """{name: [values]} of a tool's --sweep arguments ["NAME:v1,v2,...", ...], each NAME once"""
    sweep = {}
    for item in items:
        name, _, values = item.partition(":")
        if name in sweep or not values:
            raise ValueError(f"--sweep {item}: NAME:v1,v2,..., each NAME once")
        sweep[name] = [float(v) for v in values.split(",")]
    return sweep
