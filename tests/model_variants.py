"""The non-default vehicle models the GPU tests of the fused-policy, iLQR and MPPI kernels run under, defined once: the
CopterVecEnv keyword arguments of a variant, the per-env table it installs (set_vehicle_params), the hover motor value to
centre actions on, the same model for oracle.refvec.VecOracle, and the condition that makes a case under a variant
non-vacuous (the same start and action tape on the default model give another x tape in every airborne lane).

  mars_gyro           the lift thrust law in the Mars air with the rotor-gyro term (the MARS dict of the older tests)
  gyro_only           the rotor-gyro term on the live B thrust law
  vehicles            the default model, per-env M, L, Ix, Iy, Iz, maxrpm
  vehicles_mars_gyro  mars_gyro plus a per-env [12, n] table (rho and C_L rows included)
  act_f32             the float32 motor law (live model only; set_vehicle_params is refused under it)"""
import numpy as np

from jacobian_fd import VEHICLE_FIELDS, hover_action
from oracle.refcpu import AIRBORNE, DJI_PHANTOM, G, VehicleParams

MARS = dict(thrust_model="lift", rotor_gyro=True, vehicle_params={"C_L": 0.5}, world_params={"rho": 1.0})
ROWS = ("B", "D", "M", "L", "Ix", "Iy", "Iz", "Jr", "maxrpm", "G", "rho", "C_L")
VARIANTS = ("mars_gyro", "gyro_only", "vehicles", "vehicles_mars_gyro", "act_f32")
_KWARGS = {"mars_gyro": MARS, "gyro_only": dict(rotor_gyro=True), "vehicles": {}, "vehicles_mars_gyro": MARS,
           "act_f32": dict(action_arith="float32")}


def env_kwargs(name):
    """the CopterVecEnv keyword arguments of the variant (a fresh copy; None = the default model)"""
    return {} if name is None else {k: dict(v) if isinstance(v, dict) else v for k, v in _KWARGS[name].items()}


def mars_hover():
    """the motor value at which the lift law of MARS holds the DJI Phantom"""
    w = DJI_PHANTOM.maxrpm * np.pi / 30
    kl = 0.5 * 1.0 * (0.05 * DJI_PHANTOM.L * 4) * 0.5 * (DJI_PHANTOM.L / 2) ** 2 * w * w
    return np.sqrt(G * DJI_PHANTOM.M / (4 * kl))


def hover(name):
    """the hover motor value to centre actions on: the Mars value under the lift law, hover_action() otherwise (the
    per-env vehicles are spread around the vehicle these hold)"""
    return mars_hover() if name in ("mars_gyro", "vehicles_mars_gyro") else hover_action()


def vehicle_cols(rng, n):
    """per-env columns of the default model (the ranges of test_gpu_rollout_grad.py)"""
    return dict(M=rng.uniform(1.0, 2.0, n), L=rng.uniform(0.25, 0.45, n), Ix=rng.uniform(1.5, 2.5, n),
                Iy=rng.uniform(1.5, 2.5, n), Iz=rng.uniform(2.5, 3.5, n), maxrpm=rng.uniform(12000, 18000, n))


def vehicle_table(rng, n, mars):
    """a per-env [12, n] vehicle table around the DJI Phantom, in the Mars air when `mars` (the table of
    test_gpu_rollout_param_grad.py)"""
    base = dict(B=5e-3, D=2e-6, M=1.38, L=0.35, Ix=2.0, Iy=2.0, Iz=3.0, Jr=38e-4, maxrpm=15000.0, G=G,
                rho=1.0 if mars else 1.225, C_L=0.5 if mars else 0.0)
    t = np.array([np.full(n, base[k]) for k in ROWS])
    for k, lo, hi in (("M", 0.8, 1.2), ("L", 0.9, 1.1), ("Ix", 0.8, 1.2), ("Iy", 0.8, 1.2), ("Iz", 0.8, 1.2),
                      ("maxrpm", 0.9, 1.1), ("D", 0.8, 1.2), ("B", 0.9, 1.1), ("Jr", 0.8, 1.2)):
        t[ROWS.index(k)] *= rng.uniform(lo, hi, n)
    return t


def draw(name, rng, n):
    """what the variant installs per env: a dict of columns, a [12, n] table, or None (draws from rng only then)"""
    if name == "vehicles":
        return vehicle_cols(rng, n)
    if name == "vehicles_mars_gyro":
        return vehicle_table(rng, n, mars=True)
    return None


def install_same(env, installed):
    """install what install() returned for another env of the same variant (a twin)"""
    if isinstance(installed, dict):
        env.set_vehicle_params(**installed)
    elif installed is not None:
        env.set_vehicle_params(installed)
    return installed


def install(name, env, rng):
    """set_vehicle_params where the variant has a per-env table; returns what it installed (None without one)"""
    return install_same(env, draw(name, rng, env.num_envs))


def oracle_model(name, installed):
    """VecOracle's keyword arguments (vp, g, mars) of the variant with `installed`.  The oracle has the rotor-gyro term
    under the Mars model only and no float32 motor law, so gyro_only and act_f32 have no oracle."""
    if name is None:
        return dict(vp=DJI_PHANTOM, g=G, mars=None)
    if name == "mars_gyro":
        return dict(vp=DJI_PHANTOM, g=G, mars=(1.0, 0.5))
    if name == "vehicles":
        fields = {k: getattr(DJI_PHANTOM, k) for k in VEHICLE_FIELDS}
        fields.update(installed)
        return dict(vp=VehicleParams(**fields), g=G, mars=None)
    if name == "vehicles_mars_gyro":
        row = lambda k: installed[ROWS.index(k)]
        return dict(vp=VehicleParams(**{k: row(k) for k in VEHICLE_FIELDS}), g=row("G"), mars=(row("rho"), row("C_L")))
    raise ValueError("no oracle for %r" % (name,))


def stored_start(env):
    """the env's stored start as an explicit one (x, status and, where a perturbation is pending in every env, the
    pending force), for the default-model rollout below"""
    s = env.get_state()
    state = {"x": s["x"], "status": s["status"]}
    if np.all(s["flags"] & 1):
        state["force"] = s["force"]
    else:
        assert not np.any(s["flags"] & 1)
    return state


def assert_differs_from_default(name, variant_x, task, mode, substeps, state, actions):
    """The non-vacuity condition of a case under variant `name`: rollout_states(actions, state) on an env of the default
    model (for gyro_only: rotor_gyro=False) gives an x tape that differs in bits from variant_x [K, n, 12] in every
    lane that starts airborne -- were the switch ignored on both sides of the case's comparison, the tapes would be
    equal.  state is an explicit start (auto-reset is disabled: no lane resets)."""
    import gym_copter_amd
    from gpu_util import to_np
    got = np.ascontiguousarray(to_np(variant_x), dtype=np.float64)
    K, n = got.shape[:2]
    ref = gym_copter_amd.CopterVecEnv(task=task, num_envs=n, state_dtype=mode, autoreset_mode="disabled",
                                      substeps=substeps, max_steps=100000)
    try:
        assert not ref.config.rotor_gyro and ref.config.thrust_model == 0 and ref.config.action_arith == 0
        want = np.ascontiguousarray(to_np(ref.rollout_states(actions, state).x), dtype=np.float64)
    finally:
        ref.close()
    air = np.asarray(to_np(state["status"])) == AIRBORNE
    assert air.sum() >= n // 2, (name, int(air.sum()))
    same = np.all(got.view(np.uint64) == want.view(np.uint64), axis=(0, 2))
    assert not np.any(same & air), (name, "x tape equal to the default model's in %d airborne lanes"
                                    % int((same & air).sum()), np.flatnonzero(same & air)[:8])
