"""Shared by tests/test_grid_wrap_gpu.py: the diagnostic CU limit of the library (mtblx_debug_cu_limit)
as a context manager, and what a launch family starts under the limit in force
(mtblx_debug_grid_items), so that no test copies a launch constant."""
import contextlib
import os

LIMITS = (1, 3)   # 3: a stride that is no power of two


def _lib():
    import mtblx
    return mtblx.lib()


@contextlib.contextmanager
def cu_limit(n):
    """the library sizes every launch as for min(real CUs, n) compute units inside the block; the
    previous limit comes back whatever the block does"""
    L = _lib()
    prev = L.mtblx_debug_cu_limit(int(n))
    try:
        yield
    finally:
        L.mtblx_debug_cu_limit(prev)


def items(family, arg=0):
    """work items one launch of `family` (mtblx._lib.GRID_*) starts before a worker takes a second trip,
    at the limit and the routing variables in force"""
    n = int(_lib().mtblx_debug_grid_items(int(family), int(arg)))
    assert n > 0, family
    return n


def wrapped(cap, r):
    """3 * cap + r items: every worker of the launch makes at least three trips, the last one ragged"""
    n = 3 * cap + r
    assert r > 1 and 64 % r and 256 % r and n > 2 * cap   # r divides neither the wave nor the workgroup size
    return n


@contextlib.contextmanager
def env(name, value):
    """an A/B routing variable the library reads per call (None: unset)"""
    old = os.environ.get(name)
    try:
        if value is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = value
        yield
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old
