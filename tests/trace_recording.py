"""A recorder to put between a front end and its backend, and the digests its traces hold (TEST INFRASTRUCTURE): shared by the
trace tests of the Python front ends (tests/test_lt_front_trace_cpu.py, tests/test_combine_front_trace_cpu.py)."""
import hashlib

import numpy as np

_big = {}   # id -> (array, digest): key payloads are 2 MB each and are handed over on every native call


def digest(a):
    if a.size >= 1 << 18:
        hit = _big.get(id(a))
        if hit is None or hit[0] is not a:
            hit = _big[id(a)] = (a, hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16])
        return hit[1]
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def encode(x, tables=True):
    """an operand or a result as JSON; tables=False: a table of arrays is its length and its None slots, nothing is hashed"""
    if x is None or isinstance(x, (bool, int)):
        return x
    if isinstance(x, np.integer):
        return int(x)
    if isinstance(x, np.ndarray):
        return digest(x)
    if isinstance(x, (list, tuple, range)):
        if any(isinstance(v, np.ndarray) for v in x):   # a table of arrays: its length, its None slots, one digest over all
            out = {"n": len(x), "none": [i for i, v in enumerate(x) if v is None]}
            if tables:
                joined = "".join("-" if v is None else digest(v) for v in x)
                out["h"] = hashlib.sha256(joined.encode()).hexdigest()[:16]
            return out
        return [encode(v, tables) for v in x]
    raise TypeError(f"unexpected operand in a backend call: {type(x)}")


class Recorder:
    """every method call on the wrapped backend appends [name, positional operands, keyword operands, result];
    only: the entries to record (None: all), with tables=False and without the result"""

    def __init__(self, be, only=None):
        self._be, self._only, self.log = be, only, []

    def __getattr__(self, name):
        f = getattr(self._be, name)     # AttributeError for an entry the backend lacks: hasattr / getattr(.., None) see through
        if not callable(f) or (self._only is not None and name not in self._only):
            return f

        def call(*a, **k):
            r = f(*a, **k)
            if self._only is None:
                self.log.append([name, [encode(v) for v in a], {key: encode(v) for key, v in sorted(k.items())}, encode(r)])
            else:
                self.log.append([name, [encode(v, False) for v in a], {key: encode(v, False) for key, v in sorted(k.items())}])
            return r
        return call
