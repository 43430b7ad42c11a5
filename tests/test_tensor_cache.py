"""difformer_amd.tensor_cache.TensorCache: the contract every identity-keyed cache of the package shares (CSR, mixed
graphs, float32 copies, batch layouts, tiny graphs, staged operands, packed weights), checked once, on CPU tensors."""
import gc

import torch

from difformer_amd.tensor_cache import MISS, TensorCache, same_tensors, tensor_key, weak_refs


def _get(cache, tensors, extras=(), make=object):
    """What every user does: look up, build and insert on a miss."""
    v = cache.lookup(tensors, extras)
    return cache.insert(tensors, extras, make()) if v is MISS else v


def test_hit_returns_the_same_object_and_extras_are_part_of_the_key():
    c = TensorCache(4)
    a = torch.zeros(3)
    assert c.lookup((a,)) is MISS
    v = _get(c, (a,))
    assert _get(c, (a,)) is v and c.lookup((a,)) is v and len(c) == 1
    assert _get(c, (a,), (7,)) is not v and len(c) == 2
    assert c.insert((a,), (8,), None) is None and c.lookup((a,), (8,)) is None        # None is a value, not a miss


def test_in_place_edit_misses_and_the_old_version_leaves_at_the_insert():
    c = TensorCache(4)
    a = torch.zeros(3)
    v = _get(c, (a,), (1,))
    other = _get(c, (a,), (2,))
    a.add_(1)
    assert c.lookup((a,), (1,)) is MISS and len(c) == 2
    w = _get(c, (a,), (1,))
    assert w is not v and c.lookup((a,), (1,)) is w
    assert len(c) == 2 and c.values() == [other, w]           # old version of (a, extras 1) gone; other extras untouched
    _get(c, (a,), (2,))
    assert len(c) == 2


def test_none_and_a_tensor_in_the_optional_slot_are_different_keys():
    c = TensorCache(4)
    a, w = torch.zeros(3), torch.ones(3)
    plain, weighted = _get(c, (a, None)), _get(c, (a, w))
    assert plain is not weighted and len(c) == 2
    assert c.lookup((a, None)) is plain and c.lookup((a, w)) is weighted and c.lookup((a, torch.ones(3))) is MISS


def test_entries_of_freed_tensors_go_at_the_next_insert_and_at_purge_but_not_at_a_hit():
    c = TensorCache(8)
    keep, gone, w = torch.zeros(3), torch.zeros(3), torch.ones(3)
    v = _get(c, (keep, None))
    _get(c, (gone, None))
    _get(c, (keep, w))
    assert len(c) == 3
    del gone, w
    gc.collect()
    assert c.lookup((keep, None)) is v and len(c) == 3        # a hit does not walk the cache
    c.purge()
    assert len(c) == 1 and c.lookup((keep, None)) is v
    gone = torch.zeros(3)
    _get(c, (gone,))
    del gone
    gc.collect()
    assert len(c) == 2
    _get(c, (torch.zeros(2),))                                # (its own tensor is freed right after, the entry stays till later)
    assert len(c) == 2 and c.lookup((keep, None)) is v


def test_lru_order_capacity_and_reserve():
    c = TensorCache(3)
    ts = [torch.zeros(2) for _ in range(6)]
    vs = [_get(c, (t,)) for t in ts[:3]]
    assert c.lookup((ts[0],)) is vs[0]                        # refreshed: ts[1] is now the oldest
    v3 = _get(c, (ts[3],))
    assert len(c) == 3 and c.lookup((ts[1],)) is MISS and c.values() == [vs[2], vs[0], v3]
    c.reserve(5)
    _get(c, (ts[4],))
    _get(c, (ts[5],))
    assert len(c) == 5 and c.lookup((ts[2],)) is vs[2]
    _get(c, (ts[1],))
    assert len(c) == 5 and c.lookup((ts[0],)) is MISS         # ... and the bound holds at the floor
    c.reserve(0)
    _get(c, (torch.zeros(2),))
    assert len(c) <= 3
    c.clear()
    assert len(c) == 0 and c.values() == []


def test_drop_removes_every_entry_of_a_tensor():
    c = TensorCache(8)
    a, b, w = torch.zeros(3), torch.zeros(3), torch.ones(3)
    _get(c, (a, None), (1,))
    _get(c, (a, None), (2,))
    _get(c, (a, w))
    vb = _get(c, (b, w))
    c.drop(a)
    assert len(c) == 1 and c.lookup((b, w)) is vb
    c.drop(w)
    assert len(c) == 0


def test_tensors_without_a_version_are_keyed_or_never_stored():
    with torch.inference_mode():
        t = torch.zeros(3)
    assert tensor_key(t)[5] == -1
    keyed, strict = TensorCache(4, unversioned=True), TensorCache(4)
    v = _get(keyed, (t,))
    assert _get(keyed, (t,)) is v and len(keyed) == 1
    a, b = _get(strict, (t,)), _get(strict, (t,))
    assert a is not b and len(strict) == 0 and strict.lookup((t,)) is MISS
    ok = torch.zeros(3)
    _get(strict, (ok, t))                                     # one unversioned tensor among several: not stored either
    assert len(strict) == 0


def test_a_look_alike_of_a_freed_tensor_misses():
    """id, data_ptr, shape, dtype, device and version of a freed tensor can all come back with a new one: the entry is found
    under the forged key, and the weak reference (to `a`, not `b`) turns the lookup into a miss."""
    c = TensorCache(4)
    a, b = torch.zeros(3), torch.zeros(3)
    v = _get(c, (a,))
    forged = TensorCache._key(c, (a,), ())
    c._key = lambda tensors, extras: forged
    assert c.lookup((a,)) is v
    assert c.lookup((b,)) is MISS
    del c._key
    assert not same_tensors(weak_refs((a, None)), (b, None)) and not same_tensors(weak_refs((a, None)), (a, b))
    assert same_tensors(weak_refs((a, None)), (a, None))
    refs = weak_refs((a, None))
    del a
    gc.collect()
    assert not same_tensors(refs, (None, None))               # a dead reference is not a None slot
    w = _get(c, (b,))
    assert len(c) == 1 and c.lookup((b,)) is w                # ... and the insert swept the dead entry out


def test_the_packages_caches_are_tensor_caches():
    from difformer_amd import ops, staging, tiny
    for cache in (ops.csr_cache, ops.csr_cache._uniform, ops.mix_cache, ops.layout_cache, ops._F32_PARAMS, tiny.graphs,
                  staging.operands):
        assert isinstance(cache, TensorCache)
    assert [c.unversioned for c in (ops.csr_cache, ops.mix_cache, ops.layout_cache)] == [True, True, True]
    assert not any(c.unversioned for c in (ops.csr_cache._uniform, ops._F32_PARAMS, tiny.graphs, staging.operands))
    assert ops.tensor_version is not None and ops.param_key is not None
