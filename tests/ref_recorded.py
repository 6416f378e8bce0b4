"""The reference's answers to the calls tests/test_oracle_vs_ref.py makes, recorded as data.

Where oracle/_ref/libff_ref.so (the reference itself, oracle/build_ref.sh) cannot be built, the ``ref``
fixture replays tests/golden/ref_calls.npz instead.  Every call is looked up by its function name and its
arguments (arrays by dtype, shape and content hash), so a call whose inputs differ from the recorded ones
fails instead of returning an unrelated answer.

Arrays the C restatement (oracle/port.py) also computes for the same arguments are recorded as their
dtype, shape and SHA-256 only: the replay computes them with the restatement and hands them out only if
they hash to exactly the reference's recorded answer, else the call fails.  Every other answer (integers,
sizes, the points of curve_points()) is stored as it is.

Regenerate (where the reference is built):
    AMDMSM_RECORD_REF=tests/golden/ref_calls.npz python -m pytest tests/test_oracle_vs_ref.py
"""
import hashlib
import json

import numpy as np

from oracle import port
from oracle import ref as _live

# reference function -> the restatement's computation of the same answer from the same arguments
RESTATED = {name: getattr(port, name) for name in (
    "scalars_sha512", "bases_seq", "bases_r32", "multi_exp", "group_op", "scalar_mul", "fr_as_bigint", "group_consts",
    "batch_exp", "precompute_table", "disk_write", "disk_write_compressed")}
RESTATED["disk_read_compressed"] = lambda *a, **k: port.disk_read_compressed(*a, **k)[0]   # (points, bad) -> points


def _nd(a):
    a = np.ascontiguousarray(a)
    return ["nd", a.dtype.str, list(a.shape), hashlib.sha256(a.tobytes()).hexdigest()[:32]]


def call_key(name, args, kwargs):
    def norm(x):
        if isinstance(x, np.ndarray):
            return _nd(x)
        if isinstance(x, (np.integer, bool, int)):
            return int(x)
        if x is None or isinstance(x, (float, str)):
            return x
        if isinstance(x, (list, tuple)):
            return [norm(v) for v in x]
        raise TypeError(f"cannot key an argument of type {type(x).__name__}")

    key = json.dumps([name, [norm(a) for a in args], sorted((k, norm(v)) for k, v in kwargs.items())])
    return hashlib.sha256(key.encode()).hexdigest()[:32]


def _encode(x, arrays, digest):
    """digest: arrays as {"$h": dtype, shape, hash}; otherwise stored in ``arrays`` as {"$a": index}."""
    if isinstance(x, np.ndarray):
        if digest:
            return {"$h": _nd(x)}
        arrays.append(np.array(x, copy=True))
        return {"$a": len(arrays) - 1}
    if isinstance(x, tuple):
        return {"$t": [_encode(v, arrays, digest) for v in x]}
    if isinstance(x, list):
        return [_encode(v, arrays, digest) for v in x]
    if isinstance(x, dict):
        return {"$d": [[k, _encode(v, arrays, digest)] for k, v in x.items()]}
    if isinstance(x, (np.integer, np.bool_)):
        return x.item()
    return x


def _decode(x, arrays, computed=None):
    """Rebuild a recorded answer; with ``computed`` (the restatement's answer) check it against the record
    and return it."""
    if isinstance(x, dict):
        if "$h" in x:
            assert isinstance(computed, np.ndarray) and _nd(computed) == x["$h"], \
                "the restatement's answer differs from the reference's recorded one"
            return computed
        if "$a" in x:
            return arrays[x["$a"]].copy()
        if "$t" in x:
            return tuple(_decode(v, arrays, None if computed is None else computed[i]) for i, v in enumerate(x["$t"]))
        return {k: _decode(v, arrays, None if computed is None else computed[k]) for k, v in x["$d"]}
    if isinstance(x, list):
        return [_decode(v, arrays, None if computed is None else computed[i]) for i, v in enumerate(x)]
    if computed is not None:
        assert computed == x, "the restatement's answer differs from the reference's recorded one"
    return x


class RecordingRef:
    """The live reference; every call and its answer is kept for save()."""

    def __init__(self):
        self.arrays, self.index = [], {}

    def __getattr__(self, name):
        fn = getattr(_live, name)
        if not callable(fn) or name in ("available", "lib"):
            return fn

        def call(*args, **kwargs):
            key = call_key(name, args, kwargs)
            out = fn(*args, **kwargs)
            self.index[key] = _encode(out, self.arrays, name in RESTATED)   # copies: the caller may change what it got
            return out

        return call

    def save(self, path):
        np.savez_compressed(path, index=np.array(json.dumps(self.index, separators=(",", ":"))),
                            **{f"a{i}": a for i, a in enumerate(self.arrays)})


class RecordedRef:
    """Replays a recording made by RecordingRef; constants come from oracle/ref.py."""

    def __init__(self, path):
        port.build()
        with np.load(path) as z:
            self.index = json.loads(str(z["index"]))
            self.arrays = [z[f"a{i}"] for i in range(len(z.files) - 1)]

    def __getattr__(self, name):
        fn = getattr(_live, name)
        if not callable(fn):
            return fn

        def call(*args, **kwargs):
            key = call_key(name, args, kwargs)
            assert key in self.index, f"no recorded reference answer for {name}() on these inputs"
            computed = RESTATED[name](*args, **kwargs) if name in RESTATED else None
            return _decode(self.index[key], self.arrays, computed)

        return call
