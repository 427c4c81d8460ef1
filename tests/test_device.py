"""The shared host scaffolding of the wrapper classes (gpras_amd/_device.py) without a device: a stand-in for the loaded library records
the name of every call made on it."""

import ctypes as C
import gc
import os
import re

import numpy as np
import pytest

from gpras_amd import _lib
from gpras_amd._device import DeviceHandle, StageTimer, load_npz, save_npz, scoped_handle, slab_rows


class FakeLib:
    """Every attribute is a library function that logs its name and succeeds; a ``*_create`` fills the handle passed last, unless the
    name is in ``failing`` (then it answers GPRX_EINVAL and writes nothing)."""

    def __init__(self, slab=64):
        self.calls, self.failing, self.slab = [], set(), slab

    def __getattr__(self, name):
        def call(*args):
            self.calls.append(name)
            if name == "gprx_last_error":
                return b"stand-in error"
            if name in self.failing:
                return _lib.GPRX_EINVAL
            if name.endswith("_create"):
                args[-1]._obj.value = 0x1000
            if name == "gprx_pca_slab_rows":
                args[-1]._obj.value = self.slab
            return _lib.GPRX_OK

        return call


@pytest.fixture
def lib(monkeypatch):
    fake = FakeLib()
    monkeypatch.setattr(_lib, "load", lambda: fake)
    return fake


class Lazy(DeviceHandle):
    destroy_symbol = "gprx_xx_destroy"

    def __init__(self):
        super().__init__()
        self.released = 0

    def _create(self):
        _lib.check(_lib.load().gprx_xx_create(0, C.byref(self._h)))

    def _released(self):
        self.released += 1


class Eager(Lazy):
    create_on_use = False


def test_a_lazy_handle_is_created_once_at_its_first_use_and_again_after_close(lib):
    obj = Lazy()
    assert lib.calls == [] and obj._h.value is None
    assert obj.handle.value and obj.handle is obj.handle and obj.handle is obj._h
    assert lib.calls == ["gprx_xx_create"]
    obj.close()
    assert lib.calls == ["gprx_xx_create", "gprx_xx_destroy"] and obj._h.value is None
    obj.close()
    assert lib.calls == ["gprx_xx_create", "gprx_xx_destroy"]
    assert obj.handle.value
    assert lib.calls == ["gprx_xx_create", "gprx_xx_destroy", "gprx_xx_create"]
    del obj
    gc.collect()
    assert lib.calls[3:] == ["gprx_xx_destroy"]


def test_an_eager_handle_is_created_by_the_constructor_and_never_again(lib):
    obj = Eager()
    assert lib.calls == ["gprx_xx_create"] and obj._h.value
    obj.close()
    assert obj.handle.value is None and obj._h.value is None  # the library answers "null handle" to it
    assert lib.calls == ["gprx_xx_create", "gprx_xx_destroy"]
    lib.failing.add("gprx_xx_create")
    with pytest.raises(ValueError, match="stand-in error"):
        Eager()


def test_a_failed_create_leaves_nothing_to_destroy(lib):
    lib.failing.add("gprx_xx_create")
    obj = Lazy()
    with pytest.raises(ValueError, match="stand-in error"):
        obj.handle
    assert obj._h.value is None
    obj.close()
    del obj
    gc.collect()
    assert "gprx_xx_destroy" not in lib.calls and lib.calls.count("gprx_xx_create") == 1


def test_an_object_from_new_closes_and_is_collected_silently(lib):
    obj = Lazy.__new__(Lazy)
    obj.close()
    del obj
    gc.collect()
    assert lib.calls == []


def test_with_closes_on_exit_and_on_an_exception_and_the_release_hook_runs_once_per_handle(lib):
    with Lazy() as obj:
        pass
    assert lib.calls == [] and obj.released == 0  # it never had a handle
    with Lazy() as obj:
        obj.handle
    assert lib.calls == ["gprx_xx_create", "gprx_xx_destroy"] and obj.released == 1 and obj._h.value is None
    obj.close()
    assert obj.released == 1
    with pytest.raises(KeyError, match="the body's"):
        with obj:
            obj.handle
            raise KeyError("the body's")
    assert lib.calls[2:] == ["gprx_xx_create", "gprx_xx_destroy"] and obj.released == 2 and obj._h.value is None


def test_scoped_handle_destroys_after_a_body_that_raises_and_not_after_a_failed_create(lib):
    with scoped_handle(lib.gprx_yy_create, "gprx_yy_destroy", 0, 5) as h:
        assert h.value
        lib.gprx_yy_work(h)
    assert lib.calls == ["gprx_yy_create", "gprx_yy_work", "gprx_yy_destroy"]
    del lib.calls[:]
    with pytest.raises(KeyError, match="the body's"):
        with scoped_handle(lib.gprx_yy_create, "gprx_yy_destroy", 0, 5):
            raise KeyError("the body's")
    assert lib.calls == ["gprx_yy_create", "gprx_yy_destroy"]
    del lib.calls[:]
    lib.failing.add("gprx_yy_create")
    with pytest.raises(ValueError, match="stand-in error"):
        with scoped_handle(lib.gprx_yy_create, "gprx_yy_destroy", 0, 5):
            raise AssertionError("the body must not run")
    assert "gprx_yy_destroy" not in lib.calls


def test_stage_timer_sums_by_stage_in_the_order_given():
    ticks = iter([10.0, 10.5, 10.75, 12.75, 13.0, 13.25])  # seconds: the start, four laps, the end
    timer = StageTimer(("upload", "work", "download"), clock=lambda: next(ticks))
    for key in ("upload", "work", "upload", "download"):
        timer.lap(key)
    timer.link_bytes += 96
    timer.link_bytes += 32
    ms = timer.finish()
    assert list(ms) == ["upload", "work", "download", "total", "host_link_bytes"]
    assert ms == {"upload": 2500.0, "work": 250.0, "download": 250.0, "total": 3250.0, "host_link_bytes": 128}  # binary fractions: exact


@pytest.mark.parametrize("answer,most_rows,want", [(64, None, 64), (64, 10, 10), (64, 1000, 64), (0, None, 1), (0, 10, 1), (64, 0, 1)])
def test_slab_rows_clamps_to_the_rows_there_are_and_floors_at_one(lib, answer, most_rows, want):
    lib.slab = answer
    projector = Eager()
    assert slab_rows(projector, most_rows) == want
    assert lib.calls == ["gprx_xx_create", "gprx_pca_slab_rows"]


def test_npz_round_trip_keeps_the_path_and_refuses_other_files(tmp_path):
    path = tmp_path / "stored"  # no suffix, and none is appended
    arrays = {"idx": np.arange(5, dtype=np.int32), "name": np.array("wse"), "w": np.linspace(0.0, 1.0, 4)}
    save_npz(path, "fmt-1", arrays)
    assert os.listdir(tmp_path) == ["stored"]
    back = load_npz(path, "fmt-1", "thing")
    assert sorted(back) == sorted(arrays)
    for k, a in arrays.items():
        assert back[k].dtype == a.dtype and np.array_equal(back[k], a)
    with pytest.raises(ValueError, match=re.escape(f"{path}: not a thing file")):
        load_npz(path, "fmt-2", "thing")
    bare = tmp_path / "bare"
    with open(bare, "wb") as f:
        np.savez(f, idx=np.arange(5))
    with pytest.raises(ValueError, match=re.escape(f"{bare}: not a thing file")):
        load_npz(bare, "fmt-1", "thing")
    pickled = tmp_path / "pickled"
    with open(pickled, "wb") as f:
        np.savez(f, format=np.array("fmt-1"), a=np.array([{"x": 1}], dtype=object))
    with pytest.raises(ValueError, match="allow_pickle=False"):
        load_npz(pickled, "fmt-1", "thing")


def test_the_wrapper_classes_share_the_base():
    from gpras_amd.align import EventAligner
    from gpras_amd.diagnostics import FieldDiagnostics
    from gpras_amd.eigh import SymmetricEigensolver
    from gpras_amd.engine import Engine
    from gpras_amd.events import EventSelector
    from gpras_amd.preprocess import EOFProjector
    from gpras_amd.pseudo_surface import PseudoSurface
    from gpras_amd.resample import MeshResampler

    lazy, eager = (MeshResampler, PseudoSurface, EventAligner, FieldDiagnostics, EventSelector), (SymmetricEigensolver, EOFProjector, Engine)
    for cls in lazy + eager:
        assert issubclass(cls, DeviceHandle) and cls.create_on_use == (cls in lazy)
        assert "close" not in vars(cls) and "__del__" not in vars(cls) and "handle" not in vars(cls)
        assert cls.destroy_symbol in _lib.PROTOTYPES
