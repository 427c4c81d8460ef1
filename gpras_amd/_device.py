"""What every wrapper class over a family of the C ABI shares on the host: the life cycle of a library handle (``DeviceHandle``,
``scoped_handle``), the stage timer behind ``last_timings_ms`` (``StageTimer``), the projector's slab size (``slab_rows``) and the
``.npz`` container of the stored builders (``save_npz`` / ``load_npz``).  Host Python only; ``_lib`` stays the ctypes binding."""

from __future__ import annotations

import ctypes as C
import time
from contextlib import contextmanager

import numpy as np

from . import _lib
from ._lib import check


class DeviceHandle:
    """Owner of one library handle, ``self._h``.  A subclass names ``destroy_symbol`` and writes ``_create``, which fills ``self._h`` from
    the object's own attributes.  With ``create_on_use`` (the default) the handle is made at the first read of ``handle`` and again
    after a ``close()``, so building and storing the object needs no device; without it ``__init__`` makes it, a failure raises from the
    constructor, and a closed object keeps its null handle (the library answers "null handle")."""

    destroy_symbol: str
    create_on_use = True
    _h = None  # an object from ``cls.__new__`` that never ran ``__init__``: nothing to release

    def __init__(self):
        self._h = C.c_void_p()
        if not self.create_on_use:
            self._create()

    def _create(self) -> None:
        raise NotImplementedError

    def _released(self) -> None:
        """Runs when a live handle has just been destroyed: drop what was cached of its device state."""

    @property
    def handle(self):
        if self.create_on_use and not self._h.value:
            self._create()
        return self._h

    def close(self):
        if self._h is not None and self._h.value:
            getattr(_lib.load(), self.destroy_symbol)(self._h)
            self._h = C.c_void_p()
            self._released()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


@contextmanager
def scoped_handle(create, destroy_symbol: str, *args):
    """A handle for the length of one call: ``create`` is the library's create function and ``args`` its arguments before the handle it
    returns; the handle is destroyed when the block ends, also when it raises."""
    h = C.c_void_p()
    check(create(*args, C.byref(h)))
    try:
        yield h
    finally:
        getattr(_lib.load(), destroy_symbol)(h)


class StageTimer:
    """Host milliseconds by stage (every stage ends with a synchronisation of its stream) and the bytes over the host link."""

    def __init__(self, keys, clock=time.perf_counter):
        self.clock = clock
        self.ms = dict.fromkeys(keys, 0.0)
        self.start = self.mark = clock()
        self.link_bytes = 0

    def lap(self, key):
        now = self.clock()
        self.ms[key] += (now - self.mark) * 1e3
        self.mark = now

    def finish(self) -> dict[str, float]:
        """The stages in the order given, then ``"total"`` and ``"host_link_bytes"``: a ``last_timings_ms``."""
        self.ms["total"] = (self.clock() - self.start) * 1e3
        self.ms["host_link_bytes"] = self.link_bytes
        return self.ms


def slab_rows(projector, most_rows=None) -> int:
    """The rows of one slab of ``gprx_pca_transform`` for this projector, at most ``most_rows`` and at least 1."""
    rows = C.c_int64()
    check(_lib.load().gprx_pca_slab_rows(projector.handle, C.byref(rows)))
    return max(1, int(rows.value) if most_rows is None else min(int(rows.value), most_rows))


def save_npz(path, file_format: str, arrays) -> None:
    """An ``.npz`` in the convention of ``modelfile``'s portable container: plain arrays and one ``format`` string; the caller's path is
    kept as given."""
    with open(path, "wb") as f:
        np.savez(f, format=np.array(file_format), **arrays)


def load_npz(path, file_format: str, what: str) -> dict[str, np.ndarray]:
    """The arrays of ``save_npz`` (without ``format``), read with ``allow_pickle=False``; ValueError for a file of another kind."""
    with np.load(path, allow_pickle=False) as z:
        if "format" not in z.files or str(z["format"]) != file_format:
            raise ValueError(f"{path}: not a {what} file")
        return {k: z[k] for k in z.files if k != "format"}
