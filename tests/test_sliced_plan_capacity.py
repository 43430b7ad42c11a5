"""The schedule of a sliced-format build rides in the plan record (include/difformer_hip.h, "quad capacity"): bits 16-17 of
plan[0] hold the capacity - 1.  Host-side checks only (no GPU): what the two build calls accept, and that the other
readers of the record see F / 4 whatever the bits say."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    from difformer_amd import _lib
    return _lib.load()


def _measure(lib, plan, n):
    return lib.dif_sliced_measure(None, None, None, n, 0, 0, n, 64, plan, None, None, n, None, None, None, None, None, None)


def _emit(lib, plan, n):
    return lib.dif_sliced_emit(None, None, n, 0, n, 64, plan, None, None, n, None, None, None, 1, None, None)


def test_plan_carries_the_quad_capacity(lib):
    n = 5000
    plan = (ctypes.c_int32 * 8)()
    assert lib.dif_sliced_plan(n, n, 64, plan) == 0 and plan[0] == 16          # as written: capacity 1, the strict schedule
    base = list(plan)
    for bits in (0, 1):                                                         # capacity 1 and 2: accepted, next check is the pointers
        plan[0] = base[0] | bits << 16
        assert _measure(lib, plan, n) == -1 and b"null pointer" in lib.dif_last_error()
        assert _emit(lib, plan, n) == -1 and b"null pointer" in lib.dif_last_error()
    for bits in (2, 3):                                                         # capacity 3 and 4: not a schedule
        plan[0] = base[0] | bits << 16
        assert _measure(lib, plan, n) == -1 and b"quad capacity" in lib.dif_last_error()
        assert _emit(lib, plan, n) == -1 and b"quad capacity" in lib.dif_last_error()
    plan[0] = base[0] | 1 << 18                                                 # bits nobody defined
    assert _measure(lib, plan, n) == -1 and b"plan does not match" in lib.dif_last_error()
    # the product and the slice-major copy read the same geometry with or without the bits
    plan[0] = base[0] | 1 << 16
    rc = lib.dif_sliced_spmm_f32(None, None, plan, None, None, None, None, None, n, n, 0, n, 64, None, 0, 1.0, 1.0, None, 64, None, 0, None)
    assert rc == -1 and b"null pointer" in lib.dif_last_error()
