"""The sweep of every kernel instantiation (tests/test_gpu_kernel_coverage.py) once more, with every output and workspace the package
allocates poisoned and between guard bands (tests/guarded.py).  Nothing is copied: the tests, their oracles and their
tolerances are the imported ones.  What is new comes from the fixture: a store outside an allocation fails the test at
teardown, and an element that no lane wrote, or a partial sum that was never zeroed, is NaN where the oracle is finite --
which no norm-wise tolerance lets through.  Tensors the tests allocate themselves are not proxied."""
import pytest

from guarded import poisoned_allocations  # noqa: F401  (the fixture)
from test_gpu_kernel_coverage import *  # noqa: F401,F403  (tests, fixtures and the gpu mark)


@pytest.fixture(autouse=True)
def _poisoned(poisoned_allocations):
    yield
