"""The host path's per-view caches: one bounded mapping, one lookup for values derived from tensors, one table of shared constants.

Every cache of the package that is keyed by a camera, a surfel count or an image size is a `Bounded`; this module holds the only
eviction code.  There are no locks, as there were none before: each step on the underlying OrderedDict is one C call under the GIL, a
lookup that loses a race against an eviction reads as a miss, and two threads that miss on the same key both build (the later insert
stands).  That matters because autograd may run a backward on a worker thread while the main thread renders the next view.
"""
from collections import OrderedDict

import numpy as np
import torch


class Bounded:
    """A mapping that forgets its least recently used entries: at most `max_entries` of them and, with `nbytes` (entry -> bytes it pins),
    at most `max_bytes` in all -- except that the newest entry always stays.  A hit (`[]`, `get`) or an insert makes the entry the most
    recent; `bytes` is kept here, on insert, replace, pop and clear."""

    def __init__(self, max_entries, max_bytes=float("inf"), nbytes=None):
        self._d, self.max_entries, self.max_bytes, self._nbytes, self.bytes = OrderedDict(), max_entries, max_bytes, nbytes, 0

    def __len__(self):
        return len(self._d)

    def __contains__(self, key):
        return key in self._d

    def __iter__(self):
        return iter(self._d)

    def keys(self):
        return self._d.keys()

    def values(self):
        return self._d.values()

    def items(self):
        return self._d.items()

    def __getitem__(self, key):
        self._d.move_to_end(key)
        return self._d[key]

    def get(self, key, default=None):
        try:
            self._d.move_to_end(key)
            return self._d[key]
        except KeyError:
            return default

    def __setitem__(self, key, value):
        self.pop(key, None)                   # a replaced entry leaves the byte total; the new one goes to the end
        self._d[key] = value
        if self._nbytes is not None:
            self.bytes += self._nbytes(value)
        while len(self._d) > self.max_entries or (self.bytes > self.max_bytes and len(self._d) > 1):
            try:
                old = self._d.popitem(last=False)[1]      # one C call: two threads that evict at once each take an entry of their own
            except KeyError:
                break
            if self._nbytes is not None:
                self.bytes -= self._nbytes(old)

    def pop(self, key, *default):
        try:
            value = self._d.pop(key)
        except KeyError:
            if default:
                return default[0]
            raise
        if self._nbytes is not None:
            self.bytes -= self._nbytes(value)
        return value

    def clear(self):
        self._d.clear()
        self.bytes = 0


def _stamp(s):
    """What a derived value was built from, compared whole on every lookup, for the same tensor object as for another one: version
    counter, address, shape, strides, dtype and device of a tensor (an in-place write bumps the version; `t.data = other` does not, but
    moves the address), the bytes of a host array (a few dozen)."""
    if isinstance(s, torch.Tensor):
        return (s._version, s.data_ptr(), s.shape, s.stride(), s.dtype, s.device)
    return np.asarray(s).tobytes()


def derived(cache, key, sources, build):
    """`build()`, computed once per `key` and served while every one of `sources` (a tuple) still has the stamp it was built from.
    The entry holds the sources, so an address in a key or a stamp cannot be handed to another tensor while the entry lives.  The
    version is checked, never part of the key: a source written in place replaces its entry instead of leaving a dead one behind."""
    ent, now = cache.get(key), tuple(map(_stamp, sources))
    if ent is None or ent[0] != now:
        ent = cache[key] = (now, sources, build())
    return ent[2]


# Blocks of one value shared between views, READ-ONLY by convention: they stand for tensors the reference fills per render and never
# writes afterwards.  A handful per surfel count and image size; the byte bound is what a run of densification steps may leave pinned.
_CONSTANTS = Bounded(32, 256 << 20, lambda t: t.numel() * t.element_size())


def constant(shape, dtype, device, value=0):
    """The shared read-only tensor of this shape, dtype and device filled with `value` (no fill kernel per view)."""
    key = (shape, dtype, device, value)
    t = _CONSTANTS.get(key)
    if t is None:
        t = _CONSTANTS[key] = torch.full(shape, value, dtype=dtype, device=device)
    return t


def zero_leaf(like):
    """A leaf of zeros shaped like `like` whose .grad receives a gradient: a fresh tensor object over the shared zeros, whose values
    nothing reads or writes."""
    return constant(like.shape, like.dtype, like.device).detach().requires_grad_(True)
