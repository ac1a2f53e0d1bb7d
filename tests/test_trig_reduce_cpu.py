"""The device sin / cos on the host (tests/host/trig_reduce_host: gym_copter_amd/csrc/trig_reduce.h compiled as plain
C++, the library's constants and fma / rint sequence, contraction off) -- no GPU needed.

* below 8e5 the reduction is bit for bit the one it replaced (a verbatim copy in the program): sin and cos, the
  fdlibm-length and the short polynomials, >= 1e7 arguments of either sign with +-0, denormals, every k pi/2 + pi/4 for
  |k| <= 2000 with +-50 ulps around it, and 0.785, pi/4 and 8e5 with their neighbours;
* by magnitude (0.78 .. 7e11, >= 1e6 arguments of either sign each) the largest absolute error against sinl / cosl is at
  most 4 x the largest the same run measures below 8e5 -- the fold of |x| >= 8e5 costs nothing.  Measured: 2.1e-16
  against 1.8e-16 in range (FULL), 1.36e-11 against 1.36e-11 (short); the fold as it was: 5.8e-11 = 2^-34 from 1e11 on.
The table is in DESIGN.md section 3 and in dev_math.h."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host", "trig_reduce_host")
MAGNITUDES = [0.78, 3.0, 300.0, 3e4, 7.9e5, 8e5, 8.1e5, 1e8, 1e11, 7e11]
ARGS_PER_SIGN = 1000000
IDENTITY_ARGS = 10000000


@pytest.fixture(scope="module")
def report():
    p = subprocess.run([HOST, str(ARGS_PER_SIGN), str(IDENTITY_ARGS)], capture_output=True, text=True, timeout=600)
    print(p.stdout)
    rows = [ln.split() for ln in p.stdout.splitlines()]
    return p.returncode, rows


def test_the_reduction_below_8e5_is_bit_for_bit_the_one_it_replaced(report):
    _, rows = report
    ident = [r for r in rows if r and r[0] == "identity"]
    assert len(ident) == 1 and not [r for r in rows if r and r[0] == "mismatch"]
    assert int(ident[0][1]) >= IDENTITY_ARGS and int(ident[0][2]) == 0, ident


def test_accuracy_by_magnitude_stays_at_the_in_range_figure(report):
    rc, rows = report
    acc = {float(r[1]): [float(v) for v in r[2:]] for r in rows if r and r[0] == "acc"}
    assert sorted(acc) == sorted(MAGNITUDES), sorted(acc)
    in_full = max(acc[m][0] for m in MAGNITUDES if m < 8e5)
    in_short = max(acc[m][1] for m in MAGNITUDES if m < 8e5)
    said = [r for r in rows if r and r[0] == "inrange"][0]
    assert float(said[1]) == pytest.approx(in_full, rel=1e-3) and float(said[2]) == pytest.approx(in_short, rel=1e-3)
    # sanity of the in-range figures themselves: ~1 ulp of a value near 1, and the short sine's fit
    assert 5e-17 < in_full < 4e-16 and 5e-12 < in_short < 2e-11, (in_full, in_short)
    for m in MAGNITUDES:
        full, short = acc[m][:2]
        print("|x| %-8g FULL %.3e (%.2f x in range)  short %.3e (%.2f x)" % (m, full, full / in_full, short, short / in_short))
        assert full <= 4 * in_full, (m, full, in_full)
        assert short <= 4 * in_short, (m, short, in_short)
    # the fold it replaced, same arguments: what the rewrite is for (2^-34 at 1e11 and beyond)
    assert acc[1e11][2] > 1e-11 and acc[7e11][2] > 1e-11
    assert [r for r in rows if r and r[0] == "trig_reduce_host:"][0][1] == "OK" and rc == 0
