"""The branch-aware central-difference reference (tests/branch_fd.py) against closed forms the oracle implies: the
identity of LANDED and CRASHED starts, the levelled phi / theta, the clipped motor, the tilt overwrite and the
telescoping term after it, out-of-bounds over tilt, the derivative of sqrt at 0, and the stability verdict rejecting a
lane whose ground contact moves to another call under +-h.  CPU only: these pin the reference the GPU tests hold the
device gradients to (tests/test_gpu_branch_gradients.py)."""
import numpy as np

from branch_fd import LEVELLED, TOOK_OFF, event_classes, fd_rollout, fd_step, run_rollout
from jacobian_fd import hover_action
from oracle.refcpu import AIRBORNE, CRASHED, LANDED, LEVELING
from oracle.refvec import VecOracle
from rollout_fd import shaping_grad

AH = hover_action()


def _point(rng, n, z=(-20.0, -5.0)):
    x = np.zeros((12, n))
    x[0], x[2] = rng.uniform(-5, 5, (2, n))
    x[1], x[3], x[5] = rng.uniform(-1, 1, (3, n))
    x[4] = rng.uniform(*z, n)
    x[6], x[8] = rng.uniform(-0.3, 0.3, (2, n))
    x[7], x[9], x[10], x[11] = rng.uniform(-1, 1, (4, n))
    return x


def test_landed_and_crashed_starts_are_the_identity():
    """LANDED: physics skipped every step; CRASHED: every call holds.  L = sum gx_k x_k + sum gr_k r_k with
    prev_shaping = shaping(x0) differentiated: r_k = shaping(x0) - shaping(x0) + constants, so g_x0 = sum_k gx_k and
    g_actions = 0."""
    rng = np.random.default_rng(1)
    n, K = 24, 6
    for status in (LANDED, CRASHED):
        x = _point(rng, n, z=(-0.5, 0.0))
        st = np.full(n, status, np.uint8)
        a = AH * rng.uniform(0.3, 3.0, (K, n, 4))
        gx, gr = rng.standard_normal((K, n, 12)), rng.standard_normal((K, n))
        fd, ga, g0 = fd_rollout("lander3d", x, st, a, gx, gr, substeps=3)
        assert fd.keep.all()
        assert np.abs(g0 - gx.sum(axis=0).T).max() <= 1e-7
        assert np.abs(ga).max() <= 1e-7
        cl = event_classes(fd.tape, st)
        assert cl["landed_start" if status == LANDED else "crashed_start"].all()


def test_leveling_zeroes_phi_and_theta():
    """A LEVELING step overwrites phi, theta with 0: exactly 0 in those slots of g_x0, and of the step's Jacobian
    rows.  At substeps = 10 with thrust above weight the env takes off again inside the step: the action gradient of
    that step is not zero, and the phi / theta slots of g_x0 still are."""
    rng = np.random.default_rng(2)
    n = 32
    x = _point(rng, n, z=(-0.2, 0.0))
    st = np.full(n, LEVELING, np.uint8)
    fd, dx, du, rdx, rdu = fd_step("lander3d", x, st, AH * rng.uniform(0.3, 2.0, (n, 4)))
    assert fd.keep.all()
    assert not dx[:, 6].any() and not dx[:, 8].any() and not du[:, [6, 8]].any()
    assert not dx[:, :, 6].any() and not dx[:, :, 8].any() and not rdx[:, [6, 8]].any()
    K = 4
    a = AH * rng.uniform(1.05, 1.4, (K, n, 4))
    gx, gr = rng.standard_normal((K, n, 12)), rng.standard_normal((K, n))
    fd, ga, g0 = fd_rollout("lander3d", x, st, a, gx, gr, substeps=10)
    k = fd.keep
    assert k.sum() >= 3 * n // 4
    assert (fd.tape["calls"][0, 0] == LEVELLED).all() and (fd.tape["calls"][0] == TOOK_OFF).any(axis=0).all()
    assert event_classes(fd.tape, st)["leveling_takeoff"].all()
    assert not g0[6].any() and not g0[8].any()
    assert (np.abs(ga[0][k]).max(axis=1) > 1e-3).all()


def test_clipped_motor_gives_a_zero_column():
    rng = np.random.default_rng(3)
    n, K = 32, 3
    x = _point(rng, n)
    a = AH * rng.uniform(0.5, 1.5, (K, n, 4))
    a[0, :, 0] = -0.3                       # clipped at 0
    a[2, :, 2] = 1.3                        # clipped at 1: full thrust, in the last step
    gx, gr = rng.standard_normal((K, n, 12)), rng.standard_normal((K, n))
    gx[2] *= 0.01                           # (x_3 is ~100 m/s away: keep L, and its rounding, of order 1)
    gr[2] *= 0.01
    fd, ga, _ = fd_rollout("lander3d", x, np.full(n, AIRBORNE, np.uint8), a, gx, gr)
    assert fd.keep.sum() >= 3 * n // 4
    k = fd.keep
    assert not ga[0, k, 0].any() and not ga[2, k, 2].any()
    assert (np.abs(ga[0, k][:, 1:]).min(axis=1) > 0).all() and (np.abs(ga[2, k][:, [0, 1, 3]]).min(axis=1) > 0).all()
    assert event_classes(fd.tape, np.full(n, AIRBORNE))["clipped"].all()


def test_tilt_overwrites_the_reward_and_the_next_step_telescopes():
    """Step 1 ends tilted, step 2 does not.  L = r_1: reward = -penalty, no gradient at all.  L = r_2 = shaping(x_2) -
    shaping(x_1): the chain of two one-step Jacobians (fd_step at x0 and at x_1) with -grad shaping(x_1) at the
    middle.  (Leaving that term out -- treating the step after a tilt as having no prev_shaping -- is off by far more
    than the bar.)"""
    rng = np.random.default_rng(4)
    n = 160
    x = _point(rng, n)
    x[0], x[2] = rng.uniform(-3, 3, (2, n))
    x[6] = rng.uniform(0.765, 0.78, n)
    x[7] = rng.uniform(1.0, 2.0, n)
    a = AH * rng.uniform(0.8, 1.2, (2, n, 4))
    a[0, :, 0] = a[0, :, 3] = rng.uniform(0.3, 0.5, n)   # roll back hard in step 1
    st = np.full(n, AIRBORNE, np.uint8)
    fd1, ga1, g01 = fd_rollout("lander3d", x, st, a, gr=np.array([np.ones(n), np.zeros(n)]))
    tilt = fd1.tape["tilt"]
    sel = fd1.keep & tilt[1] & ~tilt[2] & ~tilt[0]
    assert sel.sum() >= 16, sel.sum()
    assert not ga1[:, sel].any() and not g01[:, sel].any()
    fd2, ga2, g02 = fd_rollout("lander3d", x, st, a, gr=np.array([np.zeros(n), np.ones(n)]))
    sel &= fd2.keep
    x1 = fd2.tape["x"][0].T
    s1, dx1, du1, _, _ = fd_step("lander3d", x, st, a[0])
    s2, dx2, du2, _, rdu2 = fd_step("lander3d", x1, fd2.tape["status"][0], a[1])
    sel &= s1.keep & s2.keep
    assert sel.sum() >= 16, sel.sum()
    x2 = fd2.tape["x"][1].T
    lam1 = np.einsum("ni,nij->nj", shaping_grad(x2).T, dx2) - shaping_grad(x1).T      # dL / dx_1
    want0 = np.einsum("ni,nij->nj", lam1, dx1)
    # (two chained differences against one: the bar is the sum of their errors, 1e-5 scaled)
    scaled = lambda g, w: np.max(np.abs(g - w) / np.maximum(1.0, np.abs(w)))       # noqa: E731
    assert scaled(g02.T[sel], want0[sel]) <= 1e-5
    assert scaled(ga2[0][sel], np.einsum("ni,nij->nj", lam1, du1)[sel]) <= 1e-5
    assert scaled(ga2[1][sel], rdu2[sel]) <= 1e-5
    skipped = np.einsum("ni,nij->nj", np.einsum("ni,nij->nj", shaping_grad(x2).T, dx2), dx1)
    assert (np.abs(skipped - want0)[sel].max(axis=1) > 1.0).all()


def test_out_of_bounds_takes_precedence_over_tilt():
    """LANDED starts (x' = x0), prev_shaping a given constant: tilted only, reward = -penalty (no gradient); out of
    bounds and tilted, reward = shaping(x0) - prev - penalty: g_x0 = grad shaping(x0)."""
    rng = np.random.default_rng(5)
    n = 32
    x = _point(rng, n, z=(-0.5, 0.0))
    x[6] = rng.choice([-1, 1], n) * rng.uniform(0.8, 1.2, n)
    oob = np.arange(n) % 2 == 0
    x[0, oob] = rng.choice([-1, 1], oob.sum()) * rng.uniform(10.5, 12, oob.sum())
    st = np.full(n, LANDED, np.uint8)
    gr = np.ones((1, n))
    fd, ga, g0 = fd_rollout("lander3d", x, st, AH * np.ones((1, n, 4)), gr=gr, prev_shaping=np.full(n, -50.0))
    assert fd.keep.all()
    assert (fd.tape["tilt"][1] == ~oob).all() and (fd.tape["oob"][1] == oob).all()
    assert not g0[:, ~oob].any() and not ga.any()
    assert np.abs(g0[:, oob] - shaping_grad(x)[:, oob]).max() <= 1e-7
    assert (np.abs(g0[:, oob]).max(axis=0) > 1.0).all()


def test_sqrt_at_zero_gives_zero_gradient():
    """A lane on the target at the origin with psi = psi' = 0 (LANDED there, or levelling there): the shaping's two
    norms are 0, and the reward gradient is 0 (the derivative of sqrt at 0 taken as 0; the central difference of |v|
    at 0 is exactly 0 too)."""
    n = 4
    x = np.zeros((12, n))
    x[6, 2:], x[8, 2:], x[7, 2:] = 0.2, -0.1, 0.5     # levelling lanes: phi, theta wiped, rates kept
    st = np.array([LANDED, LANDED, LEVELING, LEVELING], np.uint8)
    for prev in (None, np.zeros(n)):
        fd, ga, g0 = fd_rollout("lander3d", x, st, AH * np.ones((1, n, 4)), gr=np.ones((1, n)), prev_shaping=prev)
        assert fd.keep.all() and fd.tape["inside"][1].all()
        assert not g0[[0, 1, 2, 3, 4, 5, 10, 11]].any() and not ga.any()
        fd, *_, rdx, rdu = fd_step("lander3d", x, st, AH * np.ones((n, 4)))
        assert not rdx.any() and not rdu.any()


def test_contact_moving_to_another_call_is_rejected():
    """substeps = 10, a descent at 0.8 m/s reaching z = 0 exactly at the end of call 3: under +-h the contact freeze
    moves to another call, so the lane's signature differs and it is dropped; the same descent half a call earlier is
    kept."""
    n = 2
    x = np.zeros((12, n))
    x[5] = 0.8
    x[4] = [-0.0024, -0.0028]
    a = np.full((1, n, 4), 0.9 * AH)      # below hover: no take-off after the levelling call
    # put z after call 3 at 0 to the last bit: re-run the three calls and shift the start by the remainder
    for _ in range(3):
        o = VecOracle("lander3d", n, substeps=1, store_mode="float64")
        o.dt = 0.001
        o.x[:] = x
        o.status[:] = AIRBORNE
        o.prev_shaping[:] = 0.0
        for _ in range(3):
            o.step(a[0])
        x[4, 0] -= o.x[4, 0]
    gx = np.zeros((1, n, 12))
    gx[0, :, 4] = 1.0
    fd, ga, g0 = fd_rollout("lander3d", x, np.full(n, AIRBORNE, np.uint8), a, gx=gx, substeps=10)
    calls = fd.tape["calls"][0]
    assert (calls[3] == AIRBORNE * 4 + AIRBORNE).all() and (calls[4] == AIRBORNE * 4 + LEVELING).all()
    assert not fd.same[0] and not fd.keep[0]
    assert fd.keep[1]
