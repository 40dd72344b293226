"""materialrefgs_amd._cache: the bounded mapping, the lookup for values derived from tensors and the shared constants that every
per-view cache of the host path is made of.  Host code only: no GPU is needed."""
import gc
import os
import sys
import weakref

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from materialrefgs_amd._cache import Bounded, constant, derived, zero_leaf     # noqa: E402


def test_least_recently_used_entry_goes_first_and_a_hit_protects_its_entry():
    c = Bounded(3)
    for k in "abc":
        c[k] = k.upper()
    assert len(c) == 3 and "a" in c and list(c.items()) == [("a", "A"), ("b", "B"), ("c", "C")]
    assert c.get("a") == "A"                        # a hit: "a" is the most recent now, "b" the oldest
    c["d"] = "D"
    assert "b" not in c and list(c.values()) == ["C", "A", "D"]
    assert c["c"] == "C"                            # [] is a hit as well
    c["e"] = "E"
    assert "a" not in c and list(c.values()) == ["D", "C", "E"]
    c["d"] = "D2"                                   # a replacement is an insert: most recent, and nobody else leaves
    assert len(c) == 3 and list(c.values()) == ["C", "E", "D2"]
    assert c.get("zz") is None and c.get("zz", 7) == 7 and c.pop("zz", None) is None
    with pytest.raises(KeyError):
        c["zz"]
    with pytest.raises(KeyError):
        c.pop("zz")
    assert c.pop("e") == "E" and len(c) == 2
    c.clear()
    assert len(c) == 0 and "c" not in c


def test_byte_bound_and_its_total_across_insert_replace_pop_and_clear():
    c = Bounded(100, max_bytes=100, nbytes=len)
    c["a"], c["b"] = b"x" * 40, b"x" * 40
    assert c.bytes == 80
    c["a"] = b"x" * 10                              # replace: the old entry's bytes leave the total
    assert c.bytes == 50 and len(c) == 2
    c["c"] = b"x" * 60                              # 110 > 100: the least recently used ("b") goes, and that is enough
    assert "b" not in c and "a" in c and c.bytes == 70
    assert c.pop("a") == b"x" * 10 and c.bytes == 60
    assert c.pop("a", None) is None and c.bytes == 60
    c["d"] = b"x" * 500                             # larger than the bound by itself: everything else goes, the newest entry stays
    assert list(c.items()) == [("d", b"x" * 500)] and c.bytes == 500
    c["e"] = b"x"
    assert list(c.values()) == [b"x"] and c.bytes == 1
    c.clear()
    assert c.bytes == 0 and len(c) == 0
    both = Bounded(2, max_bytes=100, nbytes=len)    # both bounds hold after an insert
    for k in "abc":
        both[k] = b"x" * 10
    assert len(both) == 2 and both.bytes == 20


def _counting(value_of):
    calls = []

    def build():
        calls.append(1)
        return value_of()
    return build, calls


def test_derived_entry_is_served_for_the_same_source_and_rebuilt_after_a_write_or_for_another_tensor():
    c = Bounded(8)
    t = torch.arange(6, dtype=torch.float32)
    build, calls = _counting(lambda: t.clone())
    v0 = derived(c, "k", (t,), build)
    assert derived(c, "k", (t,), build) is v0 and derived(c, "k", (t.detach(),), build) is v0 and len(calls) == 1    # same storage, same version
    t.add_(1.0)                                     # written in place
    v1 = derived(c, "k", (t,), build)
    assert v1 is not v0 and len(calls) == 2 and torch.equal(v1, t)
    u = t.clone()                                   # equal values, another tensor
    build_u, calls_u = _counting(lambda: u.clone())
    v2 = derived(c, "k", (u,), build_u)
    assert v2 is not v1 and len(calls_u) == 1 and len(c) == 1
    a = np.arange(4.0)                              # host arrays are compared by their bytes
    build_a, calls_a = _counting(lambda: a.sum())
    assert derived(c, "h", (a, t), build_a) == 6.0 and derived(c, "h", (a.copy(), t), build_a) == 6.0 and len(calls_a) == 1
    a[0] = 1.0
    assert derived(c, "h", (a, t), build_a) == 7.0 and len(calls_a) == 2


def test_derived_entry_is_rebuilt_after_a_change_of_shape_strides_or_dtype_at_the_same_address():
    c = Bounded(8)
    m = torch.arange(16, dtype=torch.float32).reshape(4, 4)
    build, calls = _counting(object)
    first = derived(c, "k", (m,), build)
    views = [m.reshape(2, 8), m.t(), m.view(torch.int32), m.reshape(16)[:4].reshape(2, 2)]
    assert all(v.data_ptr() == m.data_ptr() and v._version == m._version for v in views)
    seen = [first]
    for v in views:
        seen.append(derived(c, "k", (v,), build))
        assert derived(c, "k", (v,), build) is seen[-1]
    assert len(calls) == 5 and len(set(map(id, seen))) == 5 and len(c) == 1


def test_derived_entry_is_rebuilt_when_the_same_tensor_object_changes_its_storage_or_layout():
    """The same Python object as a source is checked by its whole stamp, not by its version alone: `t.data = other` (what
    `module.to()` and a checkpoint load do to a Parameter) moves the address and leaves the version as it was."""
    c = Bounded(8)
    t = torch.full((4, 4), 3.0, dtype=torch.float64)
    build, calls = _counting(lambda: float(t.reshape(-1)[0]))
    assert derived(c, "k", (t,), build) == 3.0 and derived(c, "k", (t,), build) == 3.0 and len(calls) == 1
    version = t._version
    t.data = torch.full((4, 4), 5.0, dtype=torch.float64)         # another storage, same version
    assert t._version == version
    assert derived(c, "k", (t,), build) == 5.0 and derived(c, "k", (t,), build) == 5.0 and len(calls) == 2
    t.data = t.data.float()                                       # another dtype
    assert derived(c, "k", (t,), build) == 5.0 and len(calls) == 3
    t.data = t.data.t()                                           # the same address and version, other strides
    assert t._version == version
    assert derived(c, "k", (t,), build) == 5.0 and len(calls) == 4
    t.t_()                                                        # layout changed in place
    assert derived(c, "k", (t,), build) == 5.0 and len(calls) == 5
    t.resize_(2, 4)                                               # shape changed in place
    assert derived(c, "k", (t,), build) == 5.0 and derived(c, "k", (t,), build) == 5.0 and len(calls) == 6 and len(c) == 1


def test_eviction_and_iteration_go_through_the_ordered_dict():
    c = Bounded(2, max_bytes=10, nbytes=len)
    c["a"], c["b"], c["c"] = b"xx", b"xxx", b"x"
    assert list(c) == list(c.keys()) == ["b", "c"] and c.bytes == 4      # the evicted entry's bytes left the total


def test_version_is_checked_and_not_part_of_the_key():
    c = Bounded(64)
    t = torch.zeros(3)
    build, calls = _counting(lambda: float(t.sum()))
    for i in range(10):
        t.add_(1.0)
        assert derived(c, t.data_ptr(), (t,), build) == 3.0 * (i + 1)
    assert len(calls) == 10 and len(c) == 1         # ten in-place writes: ten builds, one entry


def test_entry_holds_its_source_and_an_evicted_entry_releases_it():
    c = Bounded(1)
    t = torch.ones(5)
    ref = weakref.ref(t)
    derived(c, "a", (t,), lambda: 1)
    del t
    gc.collect()
    assert ref() is not None                        # the entry pins its source: the address stays its own
    derived(c, "b", (torch.ones(2),), lambda: 2)    # evicts "a"
    gc.collect()
    assert "a" not in c and ref() is None


def test_shared_constants_are_one_object_per_key_and_the_zero_leaf_is_a_fresh_leaf_each_time():
    dev = torch.device("cpu")
    z = constant((4, 3), torch.float32, dev)
    assert constant((4, 3), torch.float32, dev) is z and constant(torch.Size((4, 3)), torch.float32, dev) is z
    assert z.shape == (4, 3) and z.dtype == torch.float32 and not z.requires_grad and float(z.abs().sum()) == 0.0
    f = constant((4, 3), torch.float32, dev, 0.01)
    assert f is not z and constant((4, 3), torch.float32, dev, 0.01) is f and bool((f == 0.01).all())
    i = constant((4, 3), torch.int32, dev)
    assert i is not z and i.dtype == torch.int32 and constant((1, 4, 3), torch.float32, dev) is not z
    like = torch.empty(4, 3)
    a, b = zero_leaf(like), zero_leaf(like)
    assert a is not b and a.is_leaf and b.is_leaf and a.requires_grad and b.requires_grad
    assert a.data_ptr() == z.data_ptr() == b.data_ptr() and a.shape == like.shape and a.dtype == like.dtype
    (a * 2.0).sum().backward()
    assert b.grad is None and bool((a.grad == 2.0).all()) and float(z.abs().sum()) == 0.0 and not z.requires_grad
