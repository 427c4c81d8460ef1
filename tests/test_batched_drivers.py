"""CPU tests of the batched forms of the drivers that mix Adam / Adadelta loops with L-BFGS-B, differential evolution or random
restarts (``optimizers.BATCHED_OPTIMIZERS``): driven by the oracle-backed stand-in of ``test_host_logic`` they leave every model
exactly as the serial driver of the same name leaves it -- variables, Z, trainable mask, evaluation count -- for several modes and
for one."""

import ctypes as C
import os
import re

import numpy as np
import pytest
from test_host_logic import BatchedOracleBackend

from gpras_amd import _lib, gpr, optimizers
from gpras_amd.synth import make_regression

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (a fresh generator per fit: the stochastic driver consumes it)
CASES = {
    "adadelta": lambda: {"max_iter": 6},
    "three-stage": lambda: {"max_iter": 4},
    "stochastic": lambda: {"n_starts": 3, "iter_initial": 2, "iter_final": 4, "rng": np.random.default_rng(5)},
    "diffential_evolution": lambda: {"popsize": 3, "max_iter": 2, "seed": 3, "adam_iter": 5, "verbose": False},
}


def _state(g):
    return [(m.w_var, m.w_len.copy(), m.w_noise, m.Z.copy(), m.n_evals, m.mask) for m in g.models]


def _same(a, b):
    assert len(a) == len(b)
    for (va, la, na, za, ea, ma), (vb, lb, nb, zb, eb, mb) in zip(a, b):
        assert va == vb and na == nb and np.array_equal(la, lb) and np.array_equal(za, zb)
        assert ea == eb and ma == mb


def _fit(x, y, method, **extra):
    g = gpr.GPRAS("RBF")
    g.fit(x, y, 7, "grid", method, **extra, **CASES[method]())
    return g


@pytest.mark.parametrize("method", list(CASES))
def test_batched_driver_equals_the_serial_driver_for_three_modes(monkeypatch, method):
    assert method in optimizers.BATCHED_OPTIMIZERS
    x, y, _ = make_regression(70, 3, n_outputs=3, n_test=0, config=8, unit=5)
    monkeypatch.setattr(gpr, "Engine", BatchedOracleBackend)
    a = _fit(x, y, method)
    assert max(a.engine.batch_sizes) == 3  # the batched route ran
    assert a.lockstep_stats["batches"] > 0 and a.lockstep_stats["evaluations"] == sum(m.n_evals for m in a.models)
    b = _fit(x, y, method, lockstep=False)
    assert not b.engine.batch_sizes
    _same(_state(a), _state(b))
    if method == "stochastic":
        # one seeded generator, drawn from up front in the serial order: the same bits every time
        _same(_state(_fit(x, y, method)), _state(a))


@pytest.mark.parametrize("method", list(CASES))
def test_batched_driver_equals_the_serial_driver_for_one_mode(monkeypatch, method):
    """GPRAS._run_optimizers sends a lone mode to the batched driver when the engine has the library loops; the stand-in has
    none, so the batched driver is called on the lone model directly."""
    x, y, _ = make_regression(70, 3, n_outputs=1, n_test=0, config=8, unit=5)
    monkeypatch.setattr(gpr, "Engine", BatchedOracleBackend)
    a = gpr.GPRAS("RBF")
    a.x, a.y = x, y
    a._init_models(x, y, 7, "grid")
    stats = {"batches": 0}
    optimizers.BATCHED_OPTIMIZERS[method](a.models, stats=stats, **CASES[method]())
    assert stats["batches"] == a.models[0].n_evals > 0
    b = _fit(x, y, method, lockstep=False)
    _same(_state(a), _state(b))


def test_adadelta_batch_is_declared_and_validates_its_handle_before_any_device_call():
    header = open(os.path.join(ROOT, "include", "gprx.h")).read()
    assert "gprx_adadelta_batch" in re.findall(r"\b(gprx_[a-z0-9_]+)\s*\(", header)
    assert "gprx_adadelta_batch" in _lib.PROTOTYPES
    lib = _lib.load()
    units = np.zeros(1, dtype=np.int32)
    theta, losses, n_evals = np.zeros(3), np.zeros(1), np.zeros(1, dtype=np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.gprx_adadelta_batch(None, 1, ptr(units), ptr(theta), None, 7, 3, ptr(losses), ptr(n_evals), None) == _lib.GPRX_EINVAL
    assert lib.gprx_last_error(None) == b"null handle"
