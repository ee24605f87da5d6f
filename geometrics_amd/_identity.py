"""The package's two answers to "have I seen this before?" ("Caches: by tensor object, by memory stamp, by device").

`ByTensor` asks "is this the tensor OBJECT I derived that table from, unchanged?": for tables built from a tensor that outlives
the call (an adjacency, a face list).  `MemoryStamp` asks "is this the MEMORY I saw, unchanged?": for hand-overs between two
launches of one step, where the same memory arrives as another tensor object.  Pure Python; both work on CPU tensors.
"""
import weakref


class ByTensor:
    """A cache keyed by one or more tensor OBJECTS and their in-place versions (+ an `extra` that has to compare equal).

    The key is the objects' identity, guarded by weak references -- never the data pointer, which the caching allocator hands to
    the next tensor of the same size.  The keys are held weakly: an entry goes when any of its key tensors dies, and the cache
    keeps none of them alive.  Values may be mutable records: a caller attaches a second derived table to the entry it has.
    versioned=False: the in-place version is not part of the key (parameters, which every step updates in place)."""

    def __init__(self, versioned=True):
        self._versioned = versioned
        self._entries = {}      # ids of the key tensors -> (weak references to them, their versions, extra, value)

    def __len__(self):
        return len(self._entries)

    def get(self, *tensors, extra=None):
        """The value stored for these very tensor objects at their present versions and this `extra`, or None."""
        hit = self._entries.get(tuple(map(id, tensors)))
        if hit is None or hit[2] != extra:
            return None
        for ref, version, t in zip(hit[0], hit[1], tensors):
            if ref() is not t or (version != t._version and self._versioned):
                return None
        return hit[3]

    def put(self, value, *tensors, extra=None):
        """Store `value` for `tensors` as they are now (replacing what was stored for them); returns `value`."""
        key = tuple(map(id, tensors))
        entries = self._entries
        refs = tuple(weakref.ref(t, lambda _r, k=key: entries.pop(k, None)) for t in tensors)
        entries[key] = (refs, tuple(t._version for t in tensors), extra, value)
        return value

    def drop(self, *tensors):
        self._entries.pop(tuple(map(id, tensors)), None)


class MemoryStamp:
    """A piece of memory as it is now: the address, element count and device of `t` and its version counter.

    The stamp HOLDS the memory (a detached tensor over it, so no autograd graph comes along): while it lives the allocator
    cannot hand the address to another tensor, which is what makes comparing addresses sound here and nowhere else.  It
    compares memory, not objects, on purpose -- the handles of utils.fan_out are distinct tensor objects over one memory --
    and element counts, not shapes (a [rows, n] reshape of a stamped [B, V, n] tensor is the same memory)."""
    __slots__ = ("held", "version")

    def __init__(self, t):
        self.held, self.version = t.detach(), t._version

    def matches(self, other):
        """Whether `other` covers the stamped memory and neither it nor the stamped tensor was written in place since."""
        held = self.held
        return (other.data_ptr() == held.data_ptr() and other.numel() == held.numel() and other.device == held.device
                and other._version == self.version and held._version == self.version)
