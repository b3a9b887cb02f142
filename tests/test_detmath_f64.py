"""Pins the f64 ln / exp pair of include/rl_detmath.h and the f64 Open01 rule of include/rl_chacha.h: both functions
within 1 ulp of 80-bit long double on every range drawn here (the bar the header states for f64 sin / cos), the special
values, a subnormal result, the two literal constants of include/rl_beta.h against the function.  CPU only.

Measured with the seed below, 2e5 points per range: rl_exp 0.80 / 0.79 / 0.81 / 0.80 ulp on [-0.35, 0.35] / [-1, 1] /
[-40, 40] / [-700, 700]; rl_log 0.80 / 0.56 / 0.74 / 0.64 ulp on [0.5, 2] / [0.9, 1.1] / exp(U[-110, 40]) /
exp(U[-700, 700])."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 200000

PROBE_C = r'''
#include <stdint.h>
#include "include/rl_beta.h"
void probe_exp(const double *x, int n, double *y) { for (int i = 0; i < n; ++i) y[i] = rl_exp(x[i]); }
void probe_log(const double *x, int n, double *y) { for (int i = 0; i < n; ++i) y[i] = rl_log(x[i]); }
double probe_open01(uint64_t w) { return rl_u64_to_open01_f64(w); }
double probe_ln4(void) { return RL_BETA_LN4; }
double probe_ln5(void) { return RL_BETA_LN5; }
'''


@pytest.fixture(scope="module")
def probe():
    d = tempfile.mkdtemp()
    src = os.path.join(d, "probe.c")
    open(src, "w").write(PROBE_C)
    so = os.path.join(d, "probe.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-std=c99", "-pedantic", "-Wall",
                           "-Wextra", "-Werror", "-I", ROOT, src, "-o", so, "-lm"])
    lib = C.CDLL(so)
    for f in (lib.probe_open01, lib.probe_ln4, lib.probe_ln5):
        f.restype = C.c_double
    return lib


def apply(fn, x):
    x = np.ascontiguousarray(x, np.float64)
    y = np.zeros_like(x)
    fn(x.ctypes.data_as(C.c_void_p), len(x), y.ctypes.data_as(C.c_void_p))
    return y


def max_ulp(y, ref):
    """the error in units of the spacing of doubles at the exact value"""
    spacing = np.spacing(np.abs(ref.astype(np.float64))).astype(np.longdouble)
    return float((np.abs(y.astype(np.longdouble) - ref) / spacing).max())


def test_long_double_is_wider_than_double():
    assert np.finfo(np.longdouble).nmant >= 63  # the reference of the two accuracy tests


@pytest.mark.parametrize("lo, hi", [(-0.35, 0.35), (-1.0, 1.0), (-40.0, 40.0), (-700.0, 700.0)])
def test_exp_accuracy(probe, lo, hi):
    x = np.random.default_rng(11).uniform(lo, hi, N)
    err = max_ulp(apply(probe.probe_exp, x), np.exp(x.astype(np.longdouble)))
    print("rl_exp on [%g, %g]: %.3f ulp" % (lo, hi, err))
    assert err <= 1.0


@pytest.mark.parametrize("name", ["[0.5, 2]", "[0.9, 1.1]", "exp(U[-110, 40])", "exp(U[-700, 700])"])
def test_log_accuracy(probe, name):
    rng = np.random.default_rng(12)
    x = {"[0.5, 2]": lambda: rng.uniform(0.5, 2.0, N), "[0.9, 1.1]": lambda: rng.uniform(0.9, 1.1, N),
         "exp(U[-110, 40])": lambda: np.exp(rng.uniform(-110.0, 40.0, N)),
         "exp(U[-700, 700])": lambda: np.exp(rng.uniform(-700.0, 700.0, N))}[name]()
    err = max_ulp(apply(probe.probe_log, x), np.log(x.astype(np.longdouble)))
    print("rl_log on %s: %.3f ulp" % (name, err))
    assert err <= 1.0


def test_special_values(probe):
    inf, nan = np.inf, np.nan
    y = apply(probe.probe_log, [0.0, -0.0, -1.0, -inf, inf, nan, 1.0, 5e-324, 2.2250738585072014e-308, 2.0])
    assert y[0] == -inf and y[1] == -inf and np.isnan(y[2]) and np.isnan(y[3]) and y[4] == inf and np.isnan(y[5])
    assert y[6] == 0.0 and not np.signbit(y[6])
    for got, x in ((y[7], 5e-324), (y[8], 2.2250738585072014e-308), (y[9], 2.0)):  # subnormals are pre-scaled
        assert abs(got - float(np.log(np.longdouble(x)))) <= np.spacing(abs(got))
    y = apply(probe.probe_exp, [nan, 709.79, 1e300, inf, -745.14, -1e300, -inf, 0.0, -0.0, 1e-300, 709.78, -745.13])
    assert np.isnan(y[0]) and y[1] == inf and y[2] == inf and y[3] == inf
    assert y[4] == 0.0 and y[5] == 0.0 and y[6] == 0.0
    assert y[7] == 1.0 and y[8] == 1.0 and y[9] == 1.0
    assert np.isfinite(y[10]) and y[10] > 1.79e308 and y[11] == 5e-324


def test_exp_subnormal_results_are_rounded_once(probe):
    """a result below 2^-1022 is within one spacing of subnormals (2^-1074) of the exact value — a second rounding of
    an already rounded 53-bit product could be off by more — and e^-740 is the double next to the exact value"""
    x = np.random.default_rng(13).uniform(-745.0, -708.4, 20000)
    y = apply(probe.probe_exp, x)
    assert np.all(y < 2.2250738585072014e-308) and np.all(y > 0.0)
    err = np.abs(y.astype(np.longdouble) - np.exp(x.astype(np.longdouble))) / np.longdouble(5e-324)
    assert float(err.max()) <= 1.0
    assert apply(probe.probe_exp, [-740.0])[0] == float(np.exp(np.longdouble(-740.0)))


def test_ln4_ln5_literals(probe):
    y = apply(probe.probe_log, [4.0, 5.0])
    assert probe.probe_ln4() == y[0] and probe.probe_ln5() == y[1]
    assert y.view(np.uint64).tolist() == [0x3FF62E42FEFA39EF, 0x3FF9C041F7ED8D33]


def test_open01_f64(probe):
    """rand 0.8.5 Open01: from_bits((w >> 12) | 0x3FF0...) - (1 - 2^-53), here in exact Python integers: the value is
    (2 m + 1) / 2^53 with m the 52 high bits"""
    for w in (0, (1 << 64) - 1, 0x8000000000000000, 0x123456789ABCDEF0):
        m = w >> 12
        want = (2 * m + 1) / float(1 << 53)  # exact: an odd integer below 2^53 over a power of two
        assert (2 * m + 1) < (1 << 53) and probe.probe_open01(C.c_uint64(w)) == want, hex(w)
    assert probe.probe_open01(C.c_uint64(0)) == 2.0 ** -53
    assert probe.probe_open01(C.c_uint64((1 << 64) - 1)) == 1.0 - 2.0 ** -53
