"""Values derived from tensors the caller owns, cached on the identity of those tensors (no imports from the package).

`forward(x, edge_index)` keeps the reference's signature, so everything built from an operand or a parameter -- the CSR
and its formats, float32 copies, packed weights, device copies of host operands -- is found again through the tensor
itself.  TensorCache is the one statement of how; its users add only what they build and when.
"""
from __future__ import annotations

import weakref
from collections import OrderedDict

MISS = object()       # what `lookup` returns when there is no entry (None is a value: "this graph is not mixed")


def tensor_version(t):
    """`t._version`, or -1 for tensors that do not track one (created under torch.inference_mode())."""
    try:
        return t._version
    except RuntimeError:
        return -1


def param_key(params):
    """Identity + version key of a list of parameters for the inference-time caches (concatenated projections,
    weight-only factors of the closed form, float32 copies), or None when a version cannot be read (inference tensors):
    the caller then rebuilds instead of caching.  NOTE: writes through `.data` (`p.data.copy_()`, EMA / weight averaging
    done on `.data`) do NOT bump the version counter -- call `model.invalidate_caches()` after such an update
    (`load_state_dict` and `.to()` / `.half()` / ... do it themselves)."""
    key = []
    for t in params:
        v = tensor_version(t)
        if v < 0:
            return None
        key.append((t.data_ptr(), v, t.dtype, t.device))
    return tuple(key)


def remembered(slot, params, build):
    """The one memo of a value derived from parameters: `slot` is None or the (key, value) pair this function returned
    last time, `build()` makes the value.  -> the pair to keep in the slot: the old one while `param_key(params)` is the
    one it was built under, else a new one, built under torch.no_grad().  An unreadable version (key None) rebuilds on
    every call.  The pair is immutable: whoever holds an old one (a captured graph) keeps the value it was built with."""
    key = param_key(params)
    if key is None or slot is None or slot[0] != key:
        import torch
        with torch.no_grad():
            slot = (key, build())
    return slot


def tensor_key(t):
    """What identifies a tensor and its contents without reading them: (id, data_ptr, shape, dtype, device, version), the
    version -1 when the tensor tracks none; None for None.  All six can come back with a NEW tensor once this one is freed:
    a holder of the key also holds `weak_refs` and asks `same_tensors`."""
    if t is None:
        return None
    try:
        return (id(t), t.data_ptr(), t.shape, t.dtype, t.device, t._version)
    except RuntimeError:
        return (id(t), t.data_ptr(), t.shape, t.dtype, t.device, -1)


def weak_refs(tensors):
    return tuple(None if t is None else weakref.ref(t) for t in tensors)


def same_tensors(refs, tensors):
    """True when `refs` (weak_refs) still resolve to exactly `tensors`, None slots included."""
    if len(refs) != len(tensors):
        return False
    for r, t in zip(refs, tensors):
        if (r is None) != (t is None) or (r is not None and r() is not t):
            return False
    return True


def _dead(refs):
    for r in refs:
        if r is not None and r() is None:
            return True
    return False


def _holds(refs, tensor):
    for r in refs:
        if r is not None and r() is tensor:
            return True
    return False


class TensorCache:
    """LRU cache of values derived from a tuple of tensors that the CALLER owns (weak references only).

    Key.     Per tensor `tensor_key` (id, data_ptr, shape, dtype, device, version); a None in an optional slot (no
             edge_weight) is part of the key; then the user's `extras`, a tuple of whatever else the value depends on.
    Hit.     An equal key AND every stored weak reference still resolving to the very tensor passed in.  Costs one key,
             one dict lookup, one weak-reference call per tensor and `move_to_end`; a hit never walks the cache, so entries
             of freed tensors stay until the next insert (or `purge`).
    Insert.  Drops the entries whose tensors have been freed, the entries of these same live tensors under the same extras
             (another version: they can never hit again), then the oldest ones beyond max(capacity, `reserve`d floor).
    Tensors without a version (made under torch.inference_mode()): `unversioned=True` keys them on -1 -- their contents
             cannot change in place --, the default never stores them (`lookup` misses, `insert` only hands the value back).
    In-place edits bump the version; writes through `.data` do not: that is what `clear` is for."""

    def __init__(self, capacity, unversioned=False):
        self.capacity, self.unversioned, self.floor = int(capacity), bool(unversioned), 0
        self.entries = OrderedDict()              # key -> (*weak_refs, value)

    def _key(self, tensors, extras):
        key = []
        for t in tensors:                         # (tensor_key written out: every hit comes through here)
            if t is None:
                key.append(None)
                continue
            try:
                v = t._version
            except RuntimeError:
                if not self.unversioned:
                    return None
                v = -1
            key.append((id(t), t.data_ptr(), t.shape, t.dtype, t.device, v))
        key.append(extras)
        return tuple(key)

    def lookup(self, tensors, extras=()):
        """The value stored for `tensors` (a tuple; None allowed in optional slots) and `extras`, or MISS."""
        key = self._key(tensors, extras)
        hit = self.entries.get(key)
        if hit is None:
            return MISS
        for r, t in zip(hit, tensors):
            if r is not None and r() is not t:
                return MISS                       # a look-alike of a freed tensor; the insert that follows replaces the entry
        self.entries.move_to_end(key)
        return hit[-1]

    def insert(self, tensors, extras, value):
        """Store `value` (-> value)."""
        key = self._key(tensors, extras)
        if key is None:
            return value
        entries = self.entries
        for k in [k for k, e in entries.items() if _dead(e[:-1]) or (k[-1] == extras and same_tensors(e[:-1], tensors))]:
            del entries[k]
        entries[key] = weak_refs(tensors) + (value,)
        bound = max(self.capacity, self.floor)
        while len(entries) > bound:
            entries.popitem(last=False)
        return value

    def purge(self):
        """Drop the entries of freed tensors now (for users whose values are large: a dead entry holds its value until the
        next insert otherwise)."""
        for k in [k for k, e in self.entries.items() if _dead(e[:-1])]:
            del self.entries[k]

    def drop(self, tensor):
        """Forget every value derived from `tensor`."""
        for k in [k for k, e in self.entries.items() if _holds(e[:-1], tensor)]:
            del self.entries[k]

    def reserve(self, n):
        """Keep room for at least n entries, whatever the capacity."""
        self.floor = max(int(n), 0)

    def values(self):
        """The values held, least recently used first."""
        return [e[-1] for e in self.entries.values()]

    def clear(self):
        self.entries.clear()

    def __len__(self):
        return len(self.entries)
