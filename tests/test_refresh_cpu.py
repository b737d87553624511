"""The host side of the values refresh, without a GPU: perturb_values
(mpg_perturb_values) against a NumPy restatement of its hash, the new symbols,
the NULL-engine argument check and the CLI's --vary-values argument errors."""
import subprocess

import numpy as np
import pytest

M64 = (1 << 64) - 1


def _mix64(z):
    """the generators' splitmix64 finaliser (problems.cpp) on Python integers"""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _restated(val, eps, seed):
    u = np.array([(_mix64(seed ^ _mix64(i)) >> 11) * 2.0 ** -52 - 1.0 for i in range(len(val))])
    return val * (1.0 + eps * u), u  # (NumPy rounds each product and sum once)


@pytest.fixture(scope="module")
def vals():
    return np.random.default_rng(11).standard_normal(1000) * 10.0 ** np.random.default_rng(12).integers(-8, 8, 1000)


def test_perturb_values_matches_the_restated_hash(mpg, vals):
    for eps, seed in ((0.3, 1), (1e-3, 2), (0.1, 2 ** 63 + 5)):
        want, u = _restated(vals, eps, seed)
        assert np.all(u >= -1.0) and np.all(u < 1.0) and u.min() < -0.9 and u.max() > 0.9
        assert np.array_equal(mpg.perturb_values(vals, eps, seed), want)


def test_perturb_values_is_deterministic_and_keyed(mpg, vals):
    a = mpg.perturb_values(vals, 0.3, 1)
    assert np.array_equal(a, mpg.perturb_values(vals, 0.3, 1))
    assert not np.array_equal(a, mpg.perturb_values(vals, 0.3, 2))  # the seed
    # the index: equal values at different places move differently, and a slice cannot be formed from index 0
    same = mpg.perturb_values(np.ones(64), 0.3, 1)
    assert len(np.unique(same)) == 64
    assert not np.array_equal(mpg.perturb_values(vals[1:], 0.3, 1), a[1:])


def test_perturb_values_bounds_and_identity(mpg, vals):
    assert np.array_equal(mpg.perturb_values(vals, 0.0, 9), vals)
    for eps in (0.3, 1e-3):
        p = mpg.perturb_values(vals, eps, 4)
        assert np.all(np.sign(p) == np.sign(vals))
        # |v| (1 - eps) <= |p| <= |v| (1 + eps), up to the two roundings of 1 + eps u and the product
        r = np.abs(p) / np.abs(vals)
        assert np.all(r >= (1 - eps) * (1 - 2 ** -51)) and np.all(r <= (1 + eps) * (1 + 2 ** -51))
    A = mpg.gen_laplace3d(4)
    assert np.array_equal(mpg.perturb_values(A, 0.1, 3), mpg.perturb_values(A.val, 0.1, 3))
    assert mpg.host_lib().mpg_perturb_values(None, 5, 0.1, 1, None) == -2
    assert mpg.host_lib().mpg_perturb_values(None, 0, 0.1, 1, None) == 0


NEW_SYMBOLS = (("solve.h", "mpg_engine_refresh_values", "host"), ("solve.h", "mpg_engine_refresh_seconds", "host"),
               ("problems.h", "mpg_perturb_values", "host"), ("capi.h", "mpg_sell_refresh_values", "hip"),
               ("arnoldi.h", "mpg_arnoldi_refresh_values", "hip"))


def test_new_symbols_are_declared_and_exported(mpg):
    declared = set(mpg.exported_capi_symbols())
    for header, name, lib in NEW_SYMBOLS:
        assert (header, name) in declared, name
        assert hasattr(mpg.host_lib() if lib == "host" else mpg.hip_lib(), name), name


def test_null_arguments_are_refused_without_a_device(mpg):
    lib, hip = mpg.host_lib(), mpg.hip_lib()
    v = np.ones(4)
    assert lib.mpg_engine_refresh_values(None, v.ctypes.data, 4, 0) == -2
    assert lib.mpg_engine_refresh_values(None, None, 0, 1) == -2
    assert lib.mpg_engine_refresh_seconds(None) == -1.0
    assert hip.mpg_sell_refresh_values(None, None, None, 0, None) == -2
    assert hip.mpg_arnoldi_refresh_values(None) == -2
    assert np.array_equal(v, np.ones(4))
    for name in ("refresh", "refresh_seconds"):
        assert hasattr(mpg.Engine, name)
    import inspect

    assert "values" in inspect.signature(mpg.Engine.solve).parameters


CLI_BASE = ["--matrix", "laplace:4", "--rlen", "10", "--orth", "cgs", "--prec", "jacobi"]


@pytest.mark.parametrize("extra", [[], ["--solves", "1"]], ids=["no --solves", "--solves 1"])
def test_cli_vary_values_needs_several_solves(mpg, extra):
    r = subprocess.run([str(mpg.CLI)] + CLI_BASE + ["--vary-values", "0.1"] + extra, capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and "--vary-values" in r.stdout and "--solves" in r.stdout, (r.stdout, r.stderr)
    assert "Doing" not in r.stdout


def test_cli_vary_values_argument_errors(mpg):
    r = subprocess.run([str(mpg.CLI)] + CLI_BASE + ["--solves", "2", "--vary-values"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1 and "Missing value for --vary-values" in r.stdout
    r = subprocess.run([str(mpg.CLI)] + CLI_BASE + ["--solves", "2", "--vary-values", "0.1", "--bpath", "b.mtx"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--bpath" in r.stdout and "Doing" not in r.stdout
