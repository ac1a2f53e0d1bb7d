"""The conditions tests/test_gpu_wide_attitudes.py rests on, checked on the float64 oracle alone (no GPU):
(a) every group of tests/attitude_points.py is populated and every wavefront is composed as stated;
(b) the central differences the derivative tests compare with are accurate where they are used: fd_jacobian at
    h = 1e-6 and at h = 3e-6 agree within BAR / 4 = 2.5e-7 on the FD point set (|yaw| <= 8 rad; measured 8.5e-8.  At
    300 rad they differ by 1.8e-6 -- the rounding of yaw +- h -- which is why the set stops at 8 rad);
(c) the yaw-periodicity tests compare what is comparable: with ONE substep the oracle's own step from psi_big and from
    its twin psi_red' agrees within 1e-15 scaled in every component but the yaw (measured 5.6e-17); with 10 substeps it
    does not (the yaw's own increments round at ulp(psi_big): 1e-5 and more), so those tests use one substep;
(d) the large-yaw forward tests can see the error of the fold they guard: 5.8e-11 rad (2^-34, the old fold's error) added
    to the twin's yaw moves the oracle's step by >= 10 x the float64 bar of 1e-13 in at least a quarter of the pairs."""
import numpy as np

import attitude_points as ap
from jacobian_fd import fd_jacobian
from oracle.refcpu import AIRBORNE

BAR = 1e-6
F64_BAR = 1e-13
OLD_FOLD_ERROR = 2.0 ** -34


def _scaled(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def test_a_groups_and_wavefronts_are_what_the_module_says():
    p = ap.points()
    x, g = p.x, p.group
    assert x.shape == (12, ap.N) and ap.N == 512
    q = ap.points()
    assert x.tobytes() == q.x.tobytes() and p.actions.tobytes() == q.actions.tobytes()       # deterministic
    wf = ap.wavefronts_in_range(x)
    assert wf[0] and wf[1] and not wf[2:].any()
    out2 = np.flatnonzero(~ap.in_range(x[:, 2 * ap.WAVE:3 * ap.WAVE]))
    assert list(out2 + 2 * ap.WAVE) == [ap.LONE_LANE]
    # the interleave: neighbours belong to different groups, every group has >= 29 lanes
    lanes = np.arange(3 * ap.WAVE, ap.N)
    assert np.all(g[lanes[:-1]] != g[lanes[1:]])
    for name in ap.WIDE_GROUPS:
        assert (g == name).sum() >= 29, name
    assert list(g[p.nonfinite]) == ["nonfinite"] * 3 and np.isposinf(x[10, p.nonfinite[0]]) and \
        np.isneginf(x[10, p.nonfinite[1]]) and np.isnan(x[10, p.nonfinite[2]])
    # yaw: every quadrant residue for either sign
    psi = x[10, g == "quadrant"]
    fn = np.rint(psi * (2 / np.pi)).astype(int)
    assert {(int(k) % 4, bool(k > 0)) for k in fn} == {(r, s) for r in range(4) for s in (False, True)}
    # the edges k pi/2 + pi/4: exact, one ulp either side, 1e-9 either side
    e = x[10, g == "edge"]
    k = np.floor(e / (np.pi / 2) + 1e-6 * np.sign(e)).astype(int)
    base = np.array([float(v) for v in (np.arange(-5, 6) * np.pi / 2 + np.pi / 4)])
    d = e - base[np.clip(np.rint((e - np.pi / 4) / (np.pi / 2)).astype(int) + 5, 0, 10)]
    assert np.all(np.abs(d) <= 1.0000001e-9) and (d == 0).any() and (np.abs(d) > 0.9e-9).any()
    assert ((d != 0) & (np.abs(d) < 1e-14)).sum() >= 4 and len(set(k)) >= 8
    y = np.abs(x[10, g == "y785"])
    assert {float(v) for v in y} == {0.785, float(np.nextafter(0.785, 1)), float(np.nextafter(0.785, 0))}
    assert (x[10, g == "y785"] < 0).any() and (x[10, g == "y785"] > 0).any()
    y = np.abs(x[10, g == "ygap"])
    assert np.all((y > 0.785) & (y < np.pi / 4))
    y = np.abs(x[10, g == "ymid"])
    assert np.all((y >= 10) & (y <= 300)) and (x[10, g == "ymid"] < 0).any()
    # the fold: every target for either sign, 8e5 exactly, pairs exact to half an ulp
    f = np.flatnonzero(g == "fold")
    big = x[10, f]
    assert (big == 8e5).any() and (big == -8e5).any()
    for t in ap.FOLD_TARGETS:
        for s in (1, -1):
            assert (np.abs(s * big - t) <= 4).any(), (t, s)
    assert ((np.abs(big) < 8e5) & (np.abs(big) > 7.8e5)).any()
    assert list(ap.pair_lanes(p)) == list(f) and np.all(np.abs(p.psi_red[f]) <= np.pi + 1e-9)
    for lane in f:
        assert ap.reduce_pair(x[10, lane], p.turns[lane]) == p.psi_red[lane]
    # roll / pitch
    for name, lo, hi in (("r0815", 0.8, 1.5), ("r231", 2.0, 3.1), ("rpi2", np.pi / 2 - 0.0201, np.pi / 2 + 0.0201)):
        m = np.maximum(np.abs(x[6, g == name]), np.abs(x[8, g == name]))
        assert np.all((m >= lo) & (m <= hi)), name
        assert (np.abs(x[6, g == name]) >= lo).any() and (np.abs(x[8, g == name]) >= lo).any(), name
    assert (np.abs(x[[6, 8]][:, g == "rpi2"]) == np.pi / 2).any()
    r = x[[6, 8]][:, g == "rgap"]
    assert np.all((np.abs(r[0]) > 0.785) & (np.abs(r[0]) < ap.TILT_LIMIT)) and (np.abs(r[1]) > 0.785).any()
    assert np.all(np.abs(x[[6, 8]][:, np.isin(g, ("quiet", "lone") + ap.YAW_GROUPS + ("nonfinite",))]) < 0.785)
    # nothing within 1e-3 of the tilt limit but the gap group; high, inside the bounds, airborne
    near = np.abs(np.abs(x[[6, 8]]) - ap.TILT_LIMIT) < 1e-3
    assert not near[:, g != "rgap"].any()
    assert np.all(x[4] <= -5) and np.all(np.abs(x[[0, 2]]) <= 4) and np.all(p.status == AIRBORNE)
    # motors: every eighth lane anywhere in 0 .. 1, the others around hover
    ah = ap.hover_motor()
    a = p.actions.astype(np.float64)
    others = np.arange(ap.N) % 8 != 0
    assert np.all((a[others] >= 0.499 * ah) & (a[others] <= 1.501 * ah)) and np.all((a >= 0) & (a <= 1))
    assert (a[::8] > 1.5 * ah).any() and (a[::8] < 0.5 * ah).any()
    # the FD set: some lanes of every group but the large yaws
    fd = ap.fd_lanes(p)
    assert {"quiet", "lone", "quadrant", "edge", "y785", "ygap", "rgap", "r0815", "rpi2", "r231"} <= set(g[fd])
    assert not {"fold", "ymid", "nonfinite"} & set(g[fd]) and fd.size >= 300
    fnq = np.rint(x[10, fd] * (2 / np.pi)).astype(int)
    assert {(int(k) % 4, bool(k > 0)) for k in fnq if k != 0} == {(r, s) for r in range(4) for s in (False, True)}


def test_a_neighbour_batch_crosses_the_bound_and_regroups_wavefronts():
    x, st, a = ap.neighbour_points()
    n, K, cut = ap.NEIGHBOUR_N, ap.NEIGHBOUR_K, ap.NEIGHBOUR_SPLIT
    assert x.shape == (12, n) and a.shape == (K, n, 4) and n == 1101 and cut == 313 and K == 12
    for substeps in (1, 3, 10):
        crossings, regrouped, wide = ap.neighbour_conditions(substeps)
        print("substeps %d: %d lane-steps cross 0.785, %d wavefronts regrouped, %.1f %% wide at the start" % (
            substeps, crossings, regrouped, 100 * wide))
        assert crossings >= 32 and regrouped >= 4 and 0.02 <= wide <= 0.06


def test_b_central_differences_are_accurate_on_the_fd_set():
    p = ap.points()
    fd = ap.fd_lanes(p)
    x, st, a = p.x[:, fd], p.status[fd], p.actions[fd].astype(np.float64)
    worst = 0.0
    for task in ("lander3d", "hover3d"):
        for substeps in (1, 10):
            j1 = fd_jacobian(task, x, st, a, substeps=substeps, h_x=1e-6, h_a=1e-6)
            j3 = fd_jacobian(task, x, st, a, substeps=substeps, h_x=3e-6, h_a=3e-6)
            for u, v in zip(j1, j3):
                worst = max(worst, float(_scaled(u, v).max()))
    print("fd_jacobian h = 1e-6 against 3e-6 on %d lanes: %.2e (bar %.1e)" % (fd.size, worst, BAR / 4))
    assert worst <= BAR / 4


def test_b_rollout_differences_are_accurate_on_the_fd_set():
    """the same for the K = 4 rollouts of the gradient test (no lane passes the tilt limit or a clip within +-h)"""
    from rollout_fd import fd_rollout_vjp
    p = ap.points()
    fd = ap.fd_lanes(p)
    x, st = p.x[:, fd], p.status[fd]
    worst = 0.0
    for task in ("lander3d", "hover3d"):
        for substeps in (1, 10):
            a, gx, gr = ap.fd_rollout_case(task, substeps)
            g1 = fd_rollout_vjp(task, x, st, a.astype(np.float64), gx=gx, gr=gr, substeps=substeps)
            g3 = fd_rollout_vjp(task, x, st, a.astype(np.float64), gx=gx, gr=gr, substeps=substeps, h_x=3e-6, h_a=3e-6)
            worst = max([worst] + [float(_scaled(u, v).max()) for u, v in zip(g1, g3)])
    print("fd_rollout_vjp h = 1e-6 against 3e-6, K = %d: %.2e (bar %.1e)" % (ap.FD_ROLLOUT_K, worst, BAR / 4))
    assert worst <= BAR / 4


def test_c_the_oracle_is_periodic_in_the_yaw_with_one_substep_only():
    d1 = max(ap.periodicity_distance(t, 1) for t in ("hover3d", "lander3d"))
    d10 = ap.periodicity_distance("hover3d", 10)
    print("oracle, psi_big against psi_red': %.2e with one substep, %.2e with ten" % (d1, d10))
    assert d1 <= 1e-15
    assert d10 > 1e-9


def test_d_the_old_folds_error_is_visible_in_one_step():
    p = ap.points()
    f, _, xr = ap.twins(p)
    a = p.actions[f].astype(np.float64)
    xe = xr.copy()
    xe[10] += OLD_FOLD_ERROR
    for substeps in (1, 10):
        n0, _, _ = ap.oracle_step("hover3d", xr, p.status[f], a, substeps)
        n1, _, _ = ap.oracle_step("hover3d", xe, p.status[f], a, substeps)
        keep = np.arange(12) != 10
        moved = _scaled(n1[keep], n0[keep]).max(axis=0)
        frac = float((moved >= 10 * F64_BAR).mean())
        print("substeps %d: 2^-34 rad of yaw moves the step by up to %.2e; >= 1e-12 in %.0f %% of %d pairs" % (
            substeps, moved.max(), 100 * frac, f.size))
        assert frac >= 0.25
