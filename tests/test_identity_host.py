"""CPU: the two identity questions of geometrics_amd._identity -- "the tensor OBJECT I built that table for, unchanged?"
(ByTensor) and "the MEMORY I saw, unchanged?" (MemoryStamp) -- on host tensors; every case is deterministic."""
import gc
import weakref

import torch

from geometrics_amd._identity import ByTensor, MemoryStamp
from geometrics_amd.backward_pass import _alias


def test_by_tensor_hits_the_same_object_and_nothing_else():
    cache = ByTensor()
    t = torch.arange(6.0)
    assert cache.get(t) is None and len(cache) == 0
    table = object()
    assert cache.put(table, t) is table
    assert cache.get(t) is table and len(cache) == 1
    same_memory = _alias(t)                     # a second tensor object over t's memory
    assert same_memory.data_ptr() == t.data_ptr() and cache.get(same_memory) is None
    same_counter = t.detach()                   # and one that shares the version counter too: still another object
    assert same_counter.data_ptr() == t.data_ptr() and same_counter._version == t._version and cache.get(same_counter) is None
    assert cache.get(t.clone()) is None
    t.add_(1.0)                                 # an in-place edit: the table was derived from other values
    assert cache.get(t) is None


def test_by_tensor_extra_has_to_compare_equal():
    cache = ByTensor()
    t = torch.zeros(4, 3, dtype=torch.int64)
    cache.put("for 7", t, extra=7)
    assert cache.get(t, extra=7) == "for 7"
    assert cache.get(t, extra=8) is None and cache.get(t) is None
    cache.put("for 8", t, extra=8)              # one entry per key: the later one replaces the earlier
    assert cache.get(t, extra=8) == "for 8" and cache.get(t, extra=7) is None and len(cache) == 1


def test_by_tensor_two_keys_miss_when_either_is_swapped_or_edited():
    cache = ByTensor()
    a, b = torch.zeros(5), torch.ones(5)
    cache.put("ab", a, b)
    assert cache.get(a, b) == "ab"
    assert cache.get(_alias(a), b) is None and cache.get(a, _alias(b)) is None
    assert cache.get(b, a) is None and cache.get(a) is None
    b.mul_(2.0)
    assert cache.get(a, b) is None
    cache.put("ab again", a, b)
    a.mul_(2.0)
    assert cache.get(a, b) is None


def test_by_tensor_holds_its_keys_weakly():
    cache = ByTensor()
    a, b, c = torch.zeros(5), torch.ones(5), torch.ones(2)
    cache.put("one", a)
    cache.put("two", b, c)
    watch = [weakref.ref(t) for t in (a, c)]
    assert len(cache) == 2
    del a
    gc.collect()
    assert len(cache) == 1 and watch[0]() is None
    del c                                       # ANY key of an entry: b is still alive
    gc.collect()
    assert len(cache) == 0 and watch[1]() is None
    assert cache.get(b, torch.ones(2)) is None


def test_by_tensor_version_blind_switch_and_drop():
    cache = ByTensor(versioned=False)
    p = torch.zeros(3, requires_grad=True)
    target = torch.zeros(3)
    cache.put(target, p)
    with torch.no_grad():
        p.add_(1.0)                             # what an optimiser does every step
    assert cache.get(p) is target
    assert cache.get(_alias(p.detach())) is None            # still the object, not the memory
    cache.drop(p)
    assert cache.get(p) is None and len(cache) == 0
    cache.drop(p)                               # (dropping what is not there is not an error)


def test_by_tensor_a_second_table_attached_to_an_entry_is_seen_by_the_next_get():
    cache = ByTensor()
    faces = torch.zeros(4, 3, dtype=torch.int64)
    cache.put(["order", None], faces)
    cache.get(faces)[1] = "faces in order"
    assert cache.get(faces) == ["order", "faces in order"] and len(cache) == 1


def test_memory_stamp_matches_the_memory_at_its_version():
    t = torch.arange(24.0).reshape(2, 3, 4)
    stamp = MemoryStamp(t)
    assert stamp.matches(t) and stamp.matches(t.detach())
    one, two = _alias(t), _alias(t)             # distinct objects over one memory, as utils.fan_out hands them out: the pooling
    assert one is not two and one._version == two._version                     # launch is given one, the block another
    assert MemoryStamp(one).matches(two) and MemoryStamp(two).matches(one)
    assert stamp.matches(t.reshape(6, 4)) and stamp.matches(t.view(-1))         # element counts, not shapes
    assert not stamp.matches(t[0]) and not stamp.matches(t[1])                 # a part of it / another address
    assert not stamp.matches(torch.arange(24.0).reshape(2, 3, 4))              # equal shape and values, elsewhere
    assert not stamp.matches(t.to(torch.float64))


def test_memory_stamp_does_not_match_after_an_in_place_edit_of_either_side():
    t = torch.zeros(2, 3, 4)
    stamp = MemoryStamp(t)
    one, two = _alias(t), _alias(t)             # (objects with version counters of their own)
    stamp_one = MemoryStamp(one)
    assert stamp_one.matches(two)
    two.add_(1.0)                               # the other side edited: its counter moves, the stamped tensor's does not
    assert not stamp_one.matches(two) and stamp_one.matches(one)
    assert stamp.matches(t) and stamp.matches(t.detach())
    t.add_(1.0)                                 # the stamped tensor itself: nothing matches any more
    assert not stamp.matches(t) and not stamp.matches(t.detach())
    fresh = MemoryStamp(t)
    assert fresh.matches(t)
    t.zero_()
    assert not fresh.matches(t)


def test_memory_stamp_holds_the_memory():
    t = torch.zeros(2, 12, 5)
    stamp = MemoryStamp(t)
    address = t.data_ptr()
    del t
    gc.collect()
    fresh = [torch.zeros(2, 12, 5) for _ in range(10)]
    assert all(f.data_ptr() != address for f in fresh)
    assert not any(stamp.matches(f) for f in fresh)


def test_memory_stamp_of_a_tensor_in_a_graph_keeps_no_graph():
    x = torch.ones(3, requires_grad=True)
    y = x * 2.0
    stamp = MemoryStamp(y)
    assert stamp.matches(y) and stamp.held.grad_fn is None and not stamp.held.requires_grad
