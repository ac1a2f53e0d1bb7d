/*
 * copterstep.h -- C ABI of libcopterstep.so: a batch ("vector env") stepper for the
 * gym-copter rigid-body hot path on AMD MI355X (gfx950).
 *
 * The upstream project (simondlevy/gym-copter) is pure Python and has no FFI layer;
 * the interface this ABI stands behind is its Gymnasium Env surface plus the public
 * methods of its Dynamics class.  Each entry point names the upstream code it
 * replaces (paths relative to the upstream checkout):
 *
 *   cs_create / cs_destroy   Lander.__init__ / _Task.__init__   envs/lander.py:25-33, envs/task.py:32-65
 *                            Dynamics.__init__                  dynamics/__init__.py:78-112
 *                            _Task.close                        envs/task.py:139-143
 *   cs_config_init           constructor defaults + constants   envs/task.py:25,32-38, envs/lander.py:17-23,
 *                                                               dynamics/__init__.py:71-76, vehicles/dji_phantom.py:9-26
 *   cs_seed                  _Task.seed                         envs/task.py:71-75
 *   cs_reset                 Lander.reset -> _Task._reset       envs/lander.py:35-37, envs/task.py:145-202
 *   cs_step / cs_step_ex     _Task.step + Lander._get_reward    envs/task.py:77-137, envs/lander.py:39-74
 *                            (+ attic hover.py:18-21, hover3d.py:32-37 for CS_TASK_HOVER3D)
 *                            which calls Dynamics.setMotors     dynamics/__init__.py:114-197,249-302
 *   cs_step_many             K x _Task.step in one launch       envs/task.py:77-137 (lander.py:40-65 loop)
 *   cs_set_motors            Dynamics.setMotors (used directly) dynamics/__init__.py:114-197
 *   cs_step_jacobian         d(_Task.step)/d(state, action)     dynamics/__init__.py:114-197,249-302, envs/task.py:77-137,
 *                            and the reward gradient            envs/lander.py:46-74 (no state written)
 *   cs_rollout_states        K x _Task.step, auto-reset off,    dynamics/__init__.py:114-197,249-302, envs/task.py:77-137,
 *                            every state kept (no state written) envs/lander.py:46-74
 *   cs_rollout_vjp           reverse-mode gradient of that      the same lines, differentiated
 *                            rollout (vector-Jacobian product)
 *   cs_rollout_*_ex          the same with a vehicle override    + the vehicle_params dict (vehicles/dji_phantom.py:9-26)
 *                            and gradients w.r.t. vehicle, force
 *   cs_rollout_mlp_states    the same rollout closed-loop       lander.py:40-65 with a policy in place of the random
 *   cs_rollout_mlp_vjp       under a fused MLP policy, and      action; the rollout lines above, differentiated
 *                            its gradient
 *   cs_rollout_mlp_vjp_ex    ... with a cotangent on the action  (a loss on the actions themselves)
 *   cs_mlp_param_grad        the gradient w.r.t. the policy's   the same loop's policy, differentiated in its weights
 *                            parameters, reduced on the device
 *   cs_rollout_lqr           the iLQR backward pass over a      the rollout lines above, differentiated (no upstream
 *                            rollout's tape                      counterpart: a second-order trajectory optimiser)
 *   cs_rollout_feedback_states  cs_rollout_states under the     lander.py:40-65 with a time-varying affine feedback
 *                            feedback that pass returns          in place of the random action
 *   cs_ilqr_box_backward     those two with the actions kept    the same lines; the box is np.clip's of task.py:91 or
 *   cs_ilqr_box_forward      inside a box (control limits)       narrower (no upstream counterpart)
 *   cs_rollout_ekf           an extended Kalman filter over     the rollout lines above and their Jacobian (no upstream
 *                            the step, K steps per env           counterpart: a state estimator)
 *   cs_rollout_rts           a Rauch-Tung-Striebel smoother     the same Jacobian at the filter's points (no upstream
 *                            over that filter's tapes            counterpart: a fixed-interval smoother)
 *   cs_rollout_pf            a bootstrap particle filter over   the rollout lines above, per particle (no upstream
 *                            the step, K steps per env           counterpart: a sampling state estimator)
 *   cs_rollout_ukf           an unscented Kalman filter over    the rollout lines above, per sigma point (no upstream
 *                            the step, K steps per env           counterpart: a derivative-free state estimator)
 *   cs_urts_smooth           an unscented Rauch-Tung-Striebel   the same points, made again from the filter's tapes
 *                            smoother over that filter's tapes   (no upstream counterpart: a fixed-interval smoother)
 *   cs_pf_smooth             a backward-simulation smoother     the rollout lines above, per taped particle (no upstream
 *                            over the particle filter's tapes    counterpart: sampled smoothed trajectories)
 *   cs_rollout_mppi_costs    P noisy copies of an action tape   lander.py:40-65 with sampled actions (no upstream
 *                            rolled out and scored              counterpart: a sampling-based trajectory optimiser)
 *   cs_rollout_mppi_update   their cost-weighted average         (the same)
 *   cs_rollout_mppi_*_ex     the same with smooth knot noise     (the same)
 *                            and a per-env temperature
 *   cs_rollout_mppi_temperature  that temperature, solved for    (the same)
 *                            an effective sample size
 *   cs_get_state             Dynamics.getState / getStatus      dynamics/__init__.py:199-207,223-225
 *   cs_export_state          the same, to device tensors        dynamics/__init__.py:199-207,223-225
 *   cs_set_state             Dynamics.setState / perturb        dynamics/__init__.py:210-217,227-229
 *   cs_set_perturbation      Dynamics.perturb (device, masked)  dynamics/__init__.py:227-229
 *   cs_episode_stats         (no upstream counterpart: batch bookkeeping)
 *   cs_comm_* / cs_allgather (no upstream counterpart: the concatenated return of a sharded batch)
 *   cs_set_altitude          _Task.set_altitude                 envs/task.py:67-69
 *   cs_obs_dim/cs_action_dim observation_space / action_space   envs/task.py:46-55 (attic variants: lander2d.py:43-50 ...)
 *   cs_set_vehicle_params    the vehicle_params dict + G        vehicles/dji_phantom.py:9-26, dynamics/__init__.py:76, envs/task.py:161
 *   cs_pid_* / cs_rollout_pid  the PID landing heuristic loop   attic/mars/pidcontrollers/__init__.py:12-146,
 *                                                               attic/mars/lander3d.py:32-36,64-87
 *   cs_rollout_random        the `--random` action loop         lander.py:40-65 (action = MOTORVAL*randn / action_space.sample())
 *   cs_serve_*               the caller's policy <-> step loop  lander.py:40-65, attic/drl/3dtest.py:44-59 (persistent env kernel)
 *   cs_get_launch_view       the same loop with the caller's policy FUSED into the K-step kernel (copterstep_rollout.h)
 *
 * Conventions
 *   - Every function returns CS_OK (0) or a negative cs_status; cs_last_error() then
 *     holds a thread-local message.  Nothing throws across this boundary.
 *   - A context owns all of its device allocations (freed by cs_destroy) and belongs to
 *     ONE HIP device (cs_config.device); the caller keeps that device current for the
 *     calls that enqueue work, as with any stream-ordered HIP library.  Pointers named *_dev are device pointers owned by the caller;
 *     pointers named *_host are host pointers.
 *   - cs_reset / cs_step / cs_step_ex / cs_step_many / cs_rollout_* / cs_set_motors only
 *     ENQUEUE work on `stream` (a hipStream_t, NULL = the null stream) and return; the
 *     caller synchronises.  They may be captured into a hipGraph: they allocate nothing
 *     and never synchronise.  cs_get_state / cs_set_state / cs_pid_get_state /
 *     cs_pid_set_state synchronise `stream`; cs_pid_configure and cs_set_vehicle_params
 *     allocate and synchronise the device (call them outside capture).
 *   - A context is not thread-safe; distinct contexts may be driven from distinct threads.
 *   - There is no CPU fallback: without a HIP device cs_create fails with CS_ERR_DEVICE.
 */
#ifndef COPTERSTEP_H
#define COPTERSTEP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history.  3: next_actions_dev ignored; Philox perturbations restored as draws by cs_set_state.
 * 4: output forms of cs_step_io (interleaved flags in every stepping entry point, packed rows in cs_step / cs_step_ex);
 *    cs_get_launch_view checks view->struct_size; cs_set_last_error; the step counter saturates at 2^S - 1 with
 *    S = bits(2 * (max_steps + 1)) (2047 at the default limit of 1000).
 * 5: the episode counter -- the Philox counter word of the reset draw and of the random policy, what cs_get_state
 *    reports and cs_episode_stats sums -- is a full 32-bit count again (ABI 4 kept 29 - S bits of it and wrapped after
 *    262 143 episodes per env at the default limit; below that number ABI 5 draws exactly what ABI 4 drew), and
 *    cs_set_state takes any uint32; cs_step_io.output_form declares the output form (packed rows are no longer
 *    inferred for a single env); cs_step_prefetch and cs_step_io.next_actions_dev (accepted and ignored since ABI 3)
 *    are gone; cs_clock_probe. */
#define CS_ABI_VERSION 5

typedef enum cs_status {
  CS_OK = 0,
  CS_ERR_ARG = -1,      /* bad argument (null pointer, bad enum, bad size) */
  CS_ERR_DEVICE = -2,   /* no usable HIP device / device ordinal out of range */
  CS_ERR_MEMORY = -3,   /* device or host allocation failed */
  CS_ERR_HIP = -4,      /* a HIP runtime call failed */
  CS_ERR_ABI = -5,      /* cs_config.struct_size / abi_version mismatch */
  CS_ERR_TIMEOUT = -6   /* served stepping: a wavefront gave up waiting (cs_serve_end / cs_serve_status) */
} cs_status;

/* 3D tasks: action [4] = the four motors; observation 10 (Lander3D: x..dtheta) or 12 (Hover3D).
 * 2D / 1D variants: the _get_motors fan-out and _get_state sub-selection of the retired variant
 * classes (attic/gym_copter/envs/lander2d.py:43-50, lander1d.py:43-48, hover2d.py:44-50,
 * hover1d.py:44-50) on the same step / reward code (task.py:94, :133):
 *   2D: action [2] -> motors (a0,a1,a1,a0), observation (y,dy,z,dz,phi,dphi)
 *   1D: action [1] -> motors (a0,a0,a0,a0), observation (z,dz) */
enum {
  CS_TASK_LANDER3D = 0,
  CS_TASK_HOVER3D = 1,
  CS_TASK_LANDER2D = 2,
  CS_TASK_LANDER1D = 3,
  CS_TASK_HOVER2D = 4,
  CS_TASK_HOVER1D = 5,
  CS_TASK_COUNT = 6
};

/* How the 12 state words are kept in HBM.  Arithmetic is float64 in registers in
 * every mode; the mode only selects the stored word and its rounding. */
enum {
  CS_STATE_F32G = 0,    /* float32 words + 5 guard bits per component, packed six
                           to a dword (default; 29 significant bits)              */
  CS_STATE_F32_RN = 1,  /* float32 words only, round-to-nearest-even              */
  CS_STATE_F64 = 2      /* float64 words                                          */
};

/* Gymnasium vector-env autoreset conventions (upstream has a single env and none). */
enum {
  CS_AUTORESET_DISABLED = 0,  /* upstream behaviour: a finished env just keeps stepping */
  CS_AUTORESET_NEXT_STEP = 1, /* the step after a done resets (action ignored, reward 0) */
  CS_AUTORESET_SAME_STEP = 2  /* reset inside the finishing step; obs = reset obs        */
};

/* Arithmetic of the motor model (dynamics/__init__.py:120-132).  The state, the rotation and the
 * integration are float64 in every case.
 *   CS_ARITH_F64: float64 -- what upstream computes for float64 / Python-float actions (lander.py:42).
 *   CS_ARITH_F32: what upstream computes when `action` is a float32 ndarray (the dtype of its
 *                 action_space, task.py:52-55): under NumPy >= 2 promotion omegas, their squares,
 *                 U1..U4 and the divisions by M, Ix, Iy, Iz all stay float32.  The two differ by
 *                 ~1e-5 relative after 1000 steps (golden trace E10). */
enum { CS_ARITH_F64 = 0, CS_ARITH_F32 = 1 };

/* Thrust law.  CS_THRUST_B: U = B * omega^2 (live model, dynamics/__init__.py:127-132).
 * CS_THRUST_LIFT: the retired Mars model's lift law, Lift_i = 0.5 * rho * S * C_L * (omega_i * L/2)^2
 * with S = 0.05 * L * 4, U1 = sum(Lift), U2 = u2(Lift), U3 = u3(Lift), U4 = D * u4(omega^2)
 * (attic/mars/dynamics/__init__.py:84-88, :135-164). */
enum { CS_THRUST_B = 0, CS_THRUST_LIFT = 1 };

/* Flight status codes, dynamics/__init__.py:65-68 */
enum { CS_STATUS_CRASHED = 0, CS_STATUS_LANDED = 1, CS_STATUS_LEVELING = 2, CS_STATUS_AIRBORNE = 3 };

typedef struct cs_config {
  uint32_t struct_size;     /* = sizeof(cs_config), set by cs_config_init */
  uint32_t abi_version;     /* = CS_ABI_VERSION */
  int32_t task;             /* CS_TASK_* */
  int32_t state_mode;       /* CS_STATE_* */
  int32_t autoreset;        /* CS_AUTORESET_* */
  int32_t substeps;         /* Dynamics.setMotors calls per env step (upstream: 1) */
  int32_t time_limit_truncates; /* 0 = upstream (step limit folded into `terminated`) */
  int32_t episode_stats;    /* 1 = keep per-env episode return on device */
  int32_t device;           /* HIP device ordinal */
  int32_t max_steps;        /* task.py:35; at most 2^20 - 3.  The step counter of an env that nobody resets saturates at
                               2^S - 1, S = bits(2 * (max_steps + 1)) (upstream's never does, task.py:130).  The episode
                               counter is a full 32-bit count whatever the limit (ABI 5). */
  int64_t num_envs;         /* environments held by this context (this shard) */
  int64_t env_id_base;      /* global id of local env 0: keys the RNG so that a batch
                               sharded over several contexts/GPUs is shard-invariant */
  uint64_t seed;
  double frames_per_second; /* task.py:25; dt = 1 / (frames_per_second * substeps) */
  /* vehicle, dji_phantom.py:9-26 */
  double B, D, M, L, Ix, Iy, Iz, Jr, maxrpm;
  /* dynamics constants, dynamics/__init__.py:71-76 */
  double G, landing_vel_x, landing_vel_y, landing_angle;
  /* task, task.py:32-38 */
  double initial_random_force, out_of_bounds_penalty, max_angle_deg, bounds, initial_altitude;
  /* lander, lander.py:17-23 */
  double target_radius, yaw_penalty_factor, xyz_penalty_factor, dz_max, dz_penalty,
      inside_radius_bonus;
  /* ---- model variants (defaults = the live upstream model) ---- */
  int32_t action_arith;     /* CS_ARITH_*: how the motor model is evaluated */
  int32_t thrust_model;     /* CS_THRUST_* */
  int32_t rotor_gyro;       /* 0 = upstream's Omega = 0 (dynamics/__init__.py:135); 1 = the retired Mars
                               model's Omega = u4(omegas) in the Jr terms (attic/mars/dynamics/__init__.py:143) */
  int32_t track_time;       /* 1 = keep Dynamics._ticks per env (dynamics/__init__.py:98, :197: the setMotors calls of
                               the episode that did not freeze on ground contact; Dynamics.getTime() = ticks * dt,
                               :219-221) and report it through cs_export_state / cs_get_state.  Selects the
                               full-featured step kernel (4 more bytes read and written per env-step). */
  double rho, C_L;          /* air density [kg/m^3] and lift coefficient of CS_THRUST_LIFT
                               (attic/mars/dynamics/__init__.py:84-88, ingenuity.py:55,72-73) */
} cs_config;

typedef struct cs_ctx cs_ctx;

/* Optional outputs of one step.  Any pointer may be NULL. */
typedef struct cs_step_io {
  const float* actions_dev;  /* [N,4] row-major, required */
  float* obs_dev;            /* [N,obs_dim] row-major (10 Lander3D / 12 Hover3D) */
  float* reward_dev;         /* [N] */
  uint8_t* terminated_dev;   /* [N] */
  uint8_t* truncated_dev;    /* [N].  INTERLEAVED FLAGS (ABI 4, every stepping entry point): truncated_dev ==
                                terminated_dev + 1 declares the two the columns of ONE [N,2] byte array
                                (terminated of env i at byte 2i, truncated at 2i+1; K-step forms: [K,N,2]) and the
                                kernels write each env's pair with one 2-byte store -- a wavefront then emits one
                                full 128-byte line instead of two half lines.  Any other pair of pointers: two
                                plain [N] arrays, as before.
                                PACKED ROWS (ABI 4; cs_step / cs_step_ex): reward_dev == obs_dev +
                                obs_dim, terminated_dev == (uint8_t*)(obs_dev + obs_dim + 1) and truncated_dev ==
                                terminated_dev + 1 declare all four outputs the columns of ONE [N, obs_dim + 2] float32
                                array: row i = {observation, reward, flags word (byte 0 terminated, byte 1 truncated,
                                bytes 2-3 zero)}, written as whole rows -- one output stream instead of three.  Note the
                                footprint: a packed row ENDS with a 4-byte flags word, two bytes past truncated_dev[i].
                                With output_form = CS_OUTPUT_AUTO the pattern is recognised for num_envs > 1 only (see
                                output_form).  The K-step, rollout and cs_serve_collect entry points refuse that pattern
                                (CS_ERR_ARG) unless the call writes ONE row in all (one env, one step: a caller's struct
                                again, written as plain arrays). */
  float* final_obs_dev;      /* [N,obs_dim]; SAME_STEP only: pre-reset observation of
                                envs that finished this step (other rows untouched) */
  /* done-mask compaction (wave ballot): ids of the envs that finished this step,
     their episode return and length, in unspecified order; *done_count_dev is
     zeroed by the library on `stream` before the kernel runs. */
  int32_t* done_count_dev;   /* [1] */
  int32_t* done_ids_dev;     /* [N] local env index */
  float* done_return_dev;    /* [N] (needs cfg.episode_stats) */
  int32_t* done_length_dev;  /* [N] */
  /* ABI 5: how the four output pointers are to be read (CS_OUTPUT_*).  CS_OUTPUT_AUTO (0, what cs_step's bare
     pointers get): interleaved flags whenever truncated_dev == terminated_dev + 1 (for one env that IS two adjacent
     bytes, so nothing can go wrong); packed rows when the pointers have that pattern AND num_envs > 1 -- four
     separate arrays of two or more envs cannot have it without overlapping, but ONE env's {obs, reward, terminated,
     truncated} may be adjacent fields of a caller's struct with no room for the flags word's last two bytes.
     CS_OUTPUT_PLAIN: never packed rows (the flags may still be interleaved).  CS_OUTPUT_PACKED_ROWS: packed rows,
     any num_envs; CS_ERR_ARG unless the pointers have the pattern. */
  uint32_t output_form;
  uint32_t reserved_;        /* 0 */
} cs_step_io;
enum { CS_OUTPUT_AUTO = 0, CS_OUTPUT_PLAIN = 1, CS_OUTPUT_PACKED_ROWS = 2 };

int cs_version(void);
const char* cs_last_error(void);
/* For code that refuses a call on the library's behalf before reaching it (include/copterstep_rollout.h: a
 * caller-side template cannot reach the library's thread-local message otherwise): sets the calling thread's
 * cs_last_error() text.  NULL clears it. */
void cs_set_last_error(const char* message);

int cs_config_init(cs_config* cfg, int task);
int cs_create(const cs_config* cfg, cs_ctx** out);
int cs_destroy(cs_ctx* ctx);   /* waits for the context's queued work; a served session still open is stopped first */

int cs_num_envs(const cs_ctx* ctx, int64_t* out);
int cs_obs_dim(const cs_ctx* ctx, int32_t* out);
int cs_action_dim(const cs_ctx* ctx, int32_t* out); /* 4, 2 (2D variants) or 1 (1D variants) */
/* Host-side settings: they take effect for launches enqueued afterwards.  A launch already
 * captured into a hipGraph carries the values of its capture time (the seed, the altitude and
 * every other cs_config value travel as kernel arguments): re-capture after changing them. */
/* cs_seed re-keys the Philox streams: both 32-bit keys are halves of splitmix64(seed), so every bit
 * of the 64-bit seed matters.  It does NOT touch the per-env episode counters (the other half of the
 * Philox counter): seeding twice with the same value does not replay the same perturbations unless
 * the counters are restored as well (cs_set_state(episode_host)).  The Philox perturbation of an episode
 * is evaluated when the physics consumes it (the first integrating step after the reset), so one that is
 * still pending when the seed changes is drawn under the NEW key. */
int cs_seed(cs_ctx* ctx, uint64_t seed);
int cs_set_altitude(cs_ctx* ctx, double altitude);
/* Reset envs with mask_dev[i] != 0 (NULL = all).  force_xyz_dev: [3,N] perturbation
 * forces in newtons to install (NULL = draw U[-F,F) with Philox2x32-10 keyed by
 * (seed, global env id, that env's episode number)).  obs_dev (nullable) receives ALL envs' observations. */
int cs_reset(cs_ctx* ctx, const uint8_t* mask_dev, const float* force_xyz_dev, float* obs_dev,
             void* stream);

/* Reset to a pose: _Task._reset(pose=(x, y, altitude, phi_deg, theta_deg), perturb=...)
 * (task.py:145, :163-176; upstream's caller is lander.py:85).  pose_dev: [5,N] float32 rows x, y,
 * altitude (up positive), roll and pitch in degrees.  perturb = 0 starts without the random force
 * (force_xyz_dev is then ignored).  Status, step counter and the Lander's initial shaping follow
 * from the pose exactly as upstream's initializing step computes them. */
int cs_reset_pose(cs_ctx* ctx, const uint8_t* mask_dev, const float* pose_dev, int32_t perturb,
                  const float* force_xyz_dev, float* obs_dev, void* stream);

int cs_step(cs_ctx* ctx, const float* actions_dev, float* obs_dev, float* reward_dev,
            uint8_t* terminated_dev, uint8_t* truncated_dev, void* stream);
int cs_step_ex(cs_ctx* ctx, const cs_step_io* io, void* stream);

/* K consecutive steps in ONE launch for action batches that are already resident (open
 * loop: recorded or random actions, shooting-style planners).  actions_dev [K,N,4];
 * obs_dev [K,N,obs_dim], reward_dev [K,N], terminated_dev / truncated_dev [K,N] (each
 * nullable).  The result is bit-identical to K calls of cs_step with actions_dev[k]; the
 * env state stays in registers between the steps instead of crossing HBM every step.
 * The optional outputs of cs_step_ex (done list, final_obs) are not produced here.
 * Fastest form (this and every cs_rollout_* entry point, up to cs_tuning.direct_rows_max_envs = 65 536 envs): whole tiles
 * (num_envs a multiple of 64), all four outputs present, the flags interleaved (truncated_dev == terminated_dev + 1, i.e.
 * one [K,N,2] byte array) -- the kernel then stores without masks, pointer tests or branches (-5 ... -9 % per step).  Any
 * other combination is served by the general instantiation; the results are the same bits either way. */
int cs_step_many(cs_ctx* ctx, int32_t num_steps, const float* actions_dev, float* obs_dev,
                 float* reward_dev, uint8_t* terminated_dev, uint8_t* truncated_dev, void* stream);

/* ---- closed-loop rollouts under the on-device PID landing heuristic -----------------------
 * Replaces, per env, the retired upstream controllers and their wiring:
 *   attic/mars/pidcontrollers/__init__.py:12-146  _PidController.compute, PositionHold /
 *                                                 Descent / AngularVelocity getDemand
 *   attic/mars/lander3d.py:32-36, :64-87          gains, heuristic(), mixer
 * Defaults of cs_pid_gains_init() are upstream's (rate 1/0/1, windup 6, 40 deg/s;
 * position 1e-5/0.1/4, target 0, windup 0.2; descent 1.15/1.33). */
enum { CS_PID_LANDER = 0, CS_PID_HOVER = 1 };
typedef struct cs_pid_gains {
  uint32_t struct_size; /* sizeof(cs_pid_gains) */
  int32_t heuristic;    /* CS_PID_LANDER: attic/mars/lander3d.py:64-87 (descent law);
                           CS_PID_HOVER: attic/mars/hover3d.py:65-92 (yaw-rate controller + the
                           altitude-hold controller of attic/mars/hover.py:23; Hover3D task only) */
  double rate_kp, rate_ki, rate_kd, rate_windup, rate_big_deg; /* AngularVelocityPidController */
  double pos_kp, pos_ki, pos_kd, pos_target, pos_windup;       /* PositionHoldPidController */
  double descent_kp, descent_kd;                               /* DescentPidController */
  double alt_kp, alt_ki, alt_kd, alt_target, alt_windup;       /* AltitudeHoldPidController (0.2, 3, 0, 5) */
} cs_pid_gains;

int cs_pid_gains_init(cs_pid_gains* gains);
/* Install gains and (first call) allocate the controller state: 24 float64 per env, zeroed =
 * freshly constructed controllers.  Synchronous; call outside stream capture.  From then on
 * cs_reset() and the auto-reset inside rollouts also restart the controllers of the envs they
 * reset. */
int cs_pid_configure(cs_ctx* ctx, const cs_pid_gains* gains);
/* Controller state <-> HOST [24,N] float64: row 4*c+f, controller c in {roll rate, pitch rate,
 * roll position (fed y), pitch position (fed x), yaw rate, altitude (the last two: hover heuristic
 * only)}, field f in {errorI, lastError, deltaError1, deltaError2}.  Synchronises `stream`. */
int cs_pid_get_state(cs_ctx* ctx, double* state_host, void* stream);
int cs_pid_set_state(cs_ctx* ctx, const double* state_host, void* stream);
/* K closed-loop steps in ONE launch: action_k = heuristic(observation returned by step k-1,
 * or the current observation for k = 0), rounded to float32, then exactly cs_step().  Outputs as
 * cs_step_many, plus actions_out_dev [K,N,4] (nullable).  Only the kernel launch is enqueued. */
int cs_rollout_pid(cs_ctx* ctx, int32_t num_steps, float* actions_out_dev, float* obs_dev,
                   float* reward_dev, uint8_t* terminated_dev, uint8_t* truncated_dev,
                   void* stream);

/* K steps in ONE launch under an on-device random policy -- the "random actions" workload
 * (lander.py --random / `env.action_space.sample()` loops) with no action tensor at all:
 * action ~ U[-1,1)^A on a 2^-15 grid from Philox2x32-10 with counter = (global env id, episode
 * number), key = hi32(splitmix64(seed)) + step counter of the episode; four
 * 16-bit uniforms per draw, the task's A of them used.  Outputs as cs_rollout_pid
 * (actions_out_dev [K,N,A], nullable). */
int cs_rollout_random(cs_ctx* ctx, int32_t num_steps, float* actions_out_dev, float* obs_dev,
                      float* reward_dev, uint8_t* terminated_dev, uint8_t* truncated_dev,
                      void* stream);

/* The caller's OWN policy fused into the K-step kernel (include/copterstep_rollout.h: a HIP source-level
 * extension point -- the policy <-> env.step() loop of lander.py:40-65 / attic/drl/3dtest.py:44-59 for any
 * policy written as a device functor).  cs_get_launch_view hands that header what a kernel instantiated in the
 * caller's translation unit is launched on: the context's folded constants and state view (opaque here; the
 * header checks their sizes against its own build of the device headers), the instantiation the library
 * itself would pick (lean / one physics call per step / per-lane row stores) and the launch shape.  The
 * pointers are into the context: valid until its configuration changes (cs_seed, cs_set_altitude,
 * cs_set_vehicle_params, cs_set_tuning) or it is destroyed.  Refused while a served session is open. */
typedef struct cs_launch_view {
  uint32_t struct_size;   /* in: sizeof(cs_launch_view), set by the caller; anything else -> CS_ERR_ABI, nothing written */
  uint32_t abi_version;   /* out: CS_ABI_VERSION of the library */
  uint32_t consts_size;   /* sizeof(cs::DevConst) / sizeof(cs::DevState) of the library's build */
  uint32_t state_size;
  int32_t task, state_mode;
  int32_t lean, one_call, direct_rows;
  uint32_t grid, block;   /* workgroups (= tiles of 64 envs), threads per workgroup (64) */
  uint32_t reserved_;
  int64_t num_envs;
  const void* consts;
  const void* state;
} cs_launch_view;
int cs_get_launch_view(cs_ctx* ctx, cs_launch_view* view);

/* Per-env vehicles and worlds (domain randomisation).  params_host: [CS_VEHICLE_ROWS, N] float64,
 * rows B, D, M, L, Ix, Iy, Iz, Jr, maxrpm -- the keys of the `vehicle_params` dict that
 * task.py:161 hands to Dynamics (dji_phantom.py:9-26; attic/mars/dynamics/ingenuity.py:46-75 for
 * another set) -- then the world: G, the gravity constant (dynamics/__init__.py:76), and rho, C_L
 * (air density and lift coefficient; read only under CS_THRUST_LIFT).  NULL returns to the
 * uniform values of cs_config.  Jr matters only with cfg.rotor_gyro (upstream multiplies it by
 * Omega = 0, :135).  Synchronous (first call allocates); call outside stream capture.  Steps then
 * read 88 more bytes per env. */
enum { CS_VEHICLE_ROWS = 12 };
int cs_set_vehicle_params(cs_ctx* ctx, const double* params_host);

/* Dynamics.perturb(force) (dynamics/__init__.py:227-229) for the envs with mask_dev[i] != 0 (NULL =
 * all): force_xyz_dev [3,N] float32 newtons becomes the pending perturbation, consumed (twice, as
 * upstream applies it) by the next integrating Dynamics.setMotors call.  Enqueue only, graph-capturable. */
int cs_set_perturbation(cs_ctx* ctx, const uint8_t* mask_dev, const float* force_xyz_dev, void* stream);

/* Running statistics of the batch as CS_EPISODE_STATS float64 values on the DEVICE (enqueue only):
 * [0] envs, [1] envs AIRBORNE, [2] sum and [3] max of the episode step counters, [4] episodes started
 * (sum over envs), [5] sum of the running episode returns (0 without cfg.episode_stats), [6] envs with a
 * non-finite (NaN / inf) state word -- upstream raises nothing on the path and lets them propagate
 * (task.py:133 only casts); this is the batch's guard counter for them. */
enum { CS_EPISODE_STATS = 7 };
int cs_episode_stats(cs_ctx* ctx, double* stats_dev, void* stream);

/* Launcher thresholds that depend on the batch size (0 = built-in default).  They select between
 * instantiations of the same step kernel and never change results.  cs_create also reads the
 * environment variables COPTERSTEP_NT_ACTION_MAX_ENVS, COPTERSTEP_NT_STATE_MIN_ENVS and
 * COPTERSTEP_DIRECT_ROWS_MAX_ENVS. */
typedef struct cs_tuning {
  uint32_t struct_size;         /* sizeof(cs_tuning) */
  uint32_t nt_action_max_envs;  /* up to this many envs the action rows are loaded non-temporally */
  uint32_t nt_state_min_envs;   /* from this many envs the state is streamed past the caches */
  uint32_t direct_rows_max_envs; /* up to this many envs the K-step kernels (cs_step_many, cs_rollout_*)
                                    store observation rows per lane instead of through the LDS transpose */
} cs_tuning;
int cs_set_tuning(cs_ctx* ctx, const cs_tuning* tuning);
int cs_get_tuning(const cs_ctx* ctx, cs_tuning* out); /* the values in effect */

/* ---- served stepping: one PERSISTENT env kernel for caller-supplied actions -------------------------
 * Replaces the caller's policy <-> env.step() loop (lander.py:40-65, attic/drl/3dtest.py:44-59) without a
 * kernel launch per env step: cs_serve_begin leaves ONE kernel running on a stream of the context's own,
 * one wavefront per tile of 64 envs with the env state in registers, for `num_steps` steps.  A step's action
 * rows reach it, and its observation / reward / flag rows leave it, as tagged 16-byte granules in two rings
 * in device memory (wire format, device-side helpers and rules: include/copterstep_serve.h).  Results are
 * bit-identical to `num_steps` calls of cs_step (both run the same step code on a register-resident env).
 *
 *   cs_serve_begin(ctx, K, ring, timeout_s, stream, &view)   zero the rings (on `stream`), fork, launch
 *   per step s = 0 .. K-1, on `stream` or on any stream ordered behind cs_serve_begin:
 *       EITHER the caller's own policy kernel speaking the wire format (copterstep_serve.h),
 *       e.g. cs_serve_policy_pid(ctx, s, stream): out(s-1) -> PID heuristic -> act(s), one launch per step
 *       OR  cs_serve_submit(ctx, s, actions_dev, stream)  +  cs_serve_collect(ctx, s, obs, ..., stream)
 *           (plain [N,A] rows in, plain rows out: one small kernel each)
 *   cs_serve_end(ctx, stream, &steps_done)                    stop word, join `stream` behind the env kernel
 *       (the stop word is raised BEHIND everything enqueued on `stream` before it: every action row published by then
 *       is still stepped; the session ends at the first step whose row is not there)
 *
 * What it costs and when it pays is measured in DESIGN.md section 8 (tools/serve_ubench.hip): a hand-off
 * between two wavefronts through device memory takes ~2 us on MI355X under this load, so a closed loop runs
 * at ~4.7 us per step against 6.5 us for policy kernel + cs_step; a caller with ONE plain kernel per step is
 * still best served by cs_step itself.
 *
 * The env kernel runs on a HIGH-PRIORITY stream of the context's own, so that it never shares a hardware
 * queue with the streams that feed it (HIP multiplexes streams onto a few hardware queues per priority level; a
 * feeder queued behind the persistent kernel would wait for it while it waits for the feeder): feed a session
 * from default-priority streams.
 * While a session is open the env state lives in its kernel's registers: every other entry point that reads or
 * writes the env state (cs_step*, cs_reset*, cs_rollout_*, cs_get_state, cs_set_state, ...) returns CS_ERR_ARG
 * until cs_serve_end.
 * While a session is open its kernel is RUNNING: a device-wide synchronisation (hipDeviceSynchronize,
 * torch.cuda.synchronize) waits for the session to end or time out; synchronise streams or events instead.
 * All env wavefronts must be resident at once: num_envs <= cs_serve_max_envs().  cs_serve_begin and
 * cs_serve_end are eager calls (they refuse a stream that is being captured: HIP may run the branches of one
 * hipGraph one after the other, and an env kernel queued in front of its own feeders would wait for ever);
 * the feeder launches of a session may be captured once -- also while no session is open: they are checked
 * against the most recent cs_serve_begin -- and replayed against every later session of the same shape
 * (num_steps, ring; tags are session-relative and cs_serve_begin zeroes the rings).  Every wait on the device is bounded by
 * timeout_s: a step whose actions never arrive ends the session with CS_ERR_TIMEOUT from cs_serve_end /
 * cs_serve_status, the env state as of the last completed step of each tile, and *steps_done = the steps
 * EVERY tile completed. */
#define CS_SERVE_TAG_INIT 0x80000000u
enum { CS_SERVE_CTRL_STOP = 0, CS_SERVE_CTRL_TIMEOUTS = 1, CS_SERVE_CTRL_SHORTFALL = 2, CS_SERVE_CTRL_MAXDONE = 3,
       CS_SERVE_CTRL_WORDS = 16 };
typedef struct cs_serve_view {
  void* act_ring;        /* [ring][tiles][act_pieces][64] x 16 B */
  void* out_ring;        /* [ring][tiles][out_pieces][64] x 16 B */
  void* out_init;        /* [tiles][out_pieces][64] x 16 B: the observation before step 0 */
  uint32_t* ctrl;        /* CS_SERVE_CTRL_WORDS control words */
  uint64_t spin_limit;   /* bound of every device-side wait, in 100 MHz ticks */
  uint32_t tiles, ring;  /* tiles = ceil(num_envs / 64); ring = a power of two */
  uint32_t act_pieces, out_pieces;  /* ceil(action_dim / 2), (obs_dim + 2) / 2 */
  uint32_t obs_dim, act_dim, num_envs, num_steps;
} cs_serve_view;
int cs_serve_max_envs(const cs_ctx* ctx, int64_t* out);
/* ring: slots per ring, a power of two in [2, 64] (0 = 4).  timeout_s <= 0 = 2 s.  view_out may be NULL. */
int cs_serve_begin(cs_ctx* ctx, int32_t num_steps, int32_t ring, double timeout_s, void* stream,
                   cs_serve_view* view_out);
/* plain action rows [N,A] of step `step` -> the action ring (waits for the ring slot, see copterstep_serve.h).
 * The feeders that WRITE into a session (cs_serve_submit, cs_serve_policy_pid*) are refused with CS_ERR_ARG when no
 * session is open and `stream` is not being captured: launched eagerly against no session they would only poll
 * until their timeout.  (Captured into a graph they may be recorded at any time and replayed against sessions.) */
int cs_serve_submit(cs_ctx* ctx, int32_t step, const float* actions_dev, void* stream);
/* wait for the outputs of step `step` (-1 = the observation before step 0) and write them as cs_step would
 * (each pointer nullable; interleaved flags as in cs_step_io).  Also valid after cs_serve_end for the steps the
 * closed session completed (its output ring is kept until the next cs_serve_begin). */
int cs_serve_collect(cs_ctx* ctx, int32_t step, float* obs_dev, float* reward_dev, uint8_t* terminated_dev,
                     uint8_t* truncated_dev, void* stream);
/* One closed-loop policy step as its own kernel: the PID heuristic of cs_pid_configure on the outputs of step
 * `step` - 1 -> the actions of `step` (controller state in the context, as cs_rollout_pid keeps it).  K of
 * these against a served session are bit-identical to cs_rollout_pid(K). */
int cs_serve_policy_pid(cs_ctx* ctx, int32_t step, void* stream);
/* The same policy for the steps [first_step, first_step + num_steps) as ONE kernel: a persistent policy kernel
 * next to the persistent env kernel -- the controllers stay in registers, and no launch is left in the loop at
 * all (what remains per step is two hand-offs and the two kernels' arithmetic).  Bit-identical to num_steps
 * launches of cs_serve_policy_pid. */
int cs_serve_policy_pid_many(cs_ctx* ctx, int32_t first_step, int32_t num_steps, void* stream);
/* Ask the env kernel to stop at the first step whose actions are not there, and order `stream` behind its
 * exit.  With steps_done != NULL it then synchronises `stream` and reports: CS_OK, or CS_ERR_TIMEOUT if a
 * wavefront gave up; *steps_done = steps completed by every tile.  With steps_done == NULL it only enqueues
 * (CS_OK): the next session can be opened right behind it, and cs_serve_status reports when asked.  Until the
 * env kernel's exit has been observed the context is "draining": every other entry point that touches the env
 * state (cs_step, cs_reset, cs_get_state, ...) first orders ITS stream behind that exit (or waits for it on the
 * host when it has no stream to order or the stream is being captured), whatever stream cs_serve_end was given. */
int cs_serve_end(cs_ctx* ctx, void* stream, int32_t* steps_done);
int cs_serve_status(cs_ctx* ctx, int32_t* steps_done_min, int32_t* steps_done_max, int32_t* timeouts);

/* ---- multi-GPU return path for C / C++ hosts: one RCCL all-gather over xGMI -------------------
 * The env batch shards trivially (no collective in stepping); the only exchange is the optional
 * concatenated return.  These wrap librccl (loaded on first use; CS_ERR_DEVICE if it is missing):
 * one communicator per process and GPU, ncclAllGather on the caller's stream (graph-capturable). */
typedef struct cs_comm cs_comm;
enum { CS_COMM_ID_BYTES = 128 };
int cs_comm_unique_id(void* id_out /* CS_COMM_ID_BYTES, from rank 0; ship it to the other ranks */);
int cs_comm_create(const void* id, int32_t world_size, int32_t rank, cs_comm** out);
int cs_comm_destroy(cs_comm* comm);
/* recv_dev [world_size * bytes] <- every rank's send_dev [bytes], in rank order */
int cs_allgather(cs_comm* comm, const void* send_dev, void* recv_dev, int64_t bytes, void* stream);

/* Diagnostic, no upstream counterpart: the shader clock this device holds under a float64 vector load.  Runs (and
 * waits for) one ~0.3 ms kernel of dependent-free v_fma_f64 on every SIMD and reports delta s_memtime / delta
 * s_memrealtime x 100 MHz, median over wavefronts, in Hz -- the clock the instruction-issue bounds of the K-step
 * kernels should be priced at on THIS device (it is typically below the peak engine clock; bench.py reports both).
 * waves_per_simd in [1, 8] wavefronts of the load per SIMD.  Synchronises `stream`. */
int cs_clock_probe(cs_ctx* ctx, int32_t waves_per_simd, double* hz_out, void* stream);
/* The PCI address of the context's device as "dddd:bb:dd.f" (NUL-terminated, len >= 16): lets a host find the
 * device's sysfs node (/sys/bus/pci/devices/<address>/hwmon/...: clocks, power, temperature) without guessing
 * which of a node's GPUs this process was given. */
int cs_device_pci_address(const cs_ctx* ctx, char* out, int32_t len);

/* Physics only: `substeps` x Dynamics.setMotors(motors[i]) on every env, raw motor
 * values (no clipping, no task logic). */
int cs_set_motors(cs_ctx* ctx, const float* motors_dev, void* stream);

/* Jacobians of one env step (dynamics/__init__.py:114-197 setMotors, :249-290 the state derivative, :292-302
 * _bodyZToInertial; envs/task.py:77-137 step, incl. the clip of :91 and the LANDED skip of :86-87; envs/lander.py:46-74
 * the reward): for every env, the derivatives of the transition cs_step(actions) would perform from the evaluation
 * point.  NOTHING of the env state is read-modified-written: the next cs_step is unaffected.
 *   dx_dev        [N,12,12]    d x' / d x   (x in upstream slot order, as cs_get_state's x)
 *   du_dev        [N,12,A]     d x' / d action, the action as cs_step receives it (before the clip; the clip's
 *                              derivative is 1 on the closed interval [0, 1] and 0 outside); A = cs_action_dim
 *   reward_dx_dev [N,12], reward_du_dev [N,A]   the gradient of the step's reward (Lander: of the shaping potential
 *                              of x', lander.py:46-57; its constants -- the |dz| > dz_max penalty, the out-of-bounds
 *                              penalty, the landing bonus, prev_shaping -- have none; a tilt (reward = -penalty), a
 *                              prev_shaping of None (reward 0), a pending reset and every Hover task give zero)
 *   branch_dev    [N] uint8    CS_JAC_* bits: which branches of the step the Jacobian is that of
 * Every output pointer may be NULL (not written); outputs are env-major and contiguous, float64 (out_dtype =
 * CS_JAC_F64) or float32 (CS_JAC_F32: the float64 values rounded).  The physics is the float64 arithmetic of the step
 * kernels, per-env vehicle table, both thrust laws and the rotor-gyro term included, chained through cfg.substeps calls
 * with the pending perturbation in the first; under action_arith = CS_ARITH_F32 it is still the float64 motor law.
 * The transition is physics + reward with auto-reset DISABLED: a termination in this step and the auto-reset behind it
 * do not enter; a NEXT_STEP reset already pending gives dx = du = 0 (the step replaces the state).
 * Evaluation point: the stored state the next cs_step starts from (x_dev == NULL: the decoded words, status, pending
 * perturbation, reset-pending flag), or the caller's x_dev [12,N] float64 + status_dev [N] (CS_STATUS_*) + optional
 * force_dev [3,N] newtons, pending (the layout of cs_get_state; no reset pending, prev_shaping taken as defined).
 * Asynchronous on `stream`.  io->struct_size must be sizeof(cs_jacobian_io) (else CS_ERR_ABI). */
typedef struct cs_jacobian_io {
  uint32_t struct_size;       /* sizeof(cs_jacobian_io) */
  uint32_t out_dtype;         /* CS_JAC_F64 / CS_JAC_F32 */
  const float* actions_dev;   /* [N,A] float32, required */
  const double* x_dev;        /* [12,N] explicit point, or NULL = the stored state */
  const uint8_t* status_dev;  /* [N] required with x_dev */
  const double* force_dev;    /* [3,N] newtons, optional with x_dev (NULL = no perturbation pending) */
  void* dx_dev;
  void* du_dev;
  void* reward_dx_dev;
  void* reward_du_dev;
  uint8_t* branch_dev;
} cs_jacobian_io;
enum { CS_JAC_F64 = 0, CS_JAC_F32 = 1 };
enum {
  CS_JAC_INTEGRATED = 1,  /* at least one setMotors call integrated */
  CS_JAC_LANDED = 2,      /* LANDED at the start: physics skipped, dx = I, du = 0 */
  CS_JAC_CONTACT = 4,     /* a call froze on ground contact (:162-177): identity rows from there on */
  CS_JAC_LEVELING = 8,    /* a call levelled the wings: the phi, theta rows are zero */
  CS_JAC_CRASHED = 16,    /* a call found the env CRASHED: it only ticks */
  CS_JAC_RESET = 32,      /* a NEXT_STEP reset is pending: dx = du = 0 */
  CS_JAC_CLIPPED = 64     /* some motor value was outside [0, 1]: its columns are zero */
};
int cs_step_jacobian(cs_ctx* ctx, const cs_jacobian_io* io, void* stream);

/* Differentiable K-step rollouts (dynamics/__init__.py:114-197 setMotors, :249-302 the state derivative and
 * _bodyZToInertial; envs/task.py:77-137 step; envs/lander.py:46-74 the reward).  A rollout is the pure function "K calls
 * of cs_step on this env with auto-reset DISABLED": NOTHING of the env state is written -- no words, counters, episode
 * numbers, prev_shaping, statistics or RNG position.
 *
 * cs_rollout_states (forward): from the start point, step k = 1..K takes actions_dev[k-1] and writes
 *   x_dev          [K,N,12] float64  the decoded stored state after step k, in upstream slot order (cs_get_state's x
 *                                    slots; in the float32 storage modes the words cs_get_state would report)
 *   reward_dev     [K,N]    float64  the reward before cs_step rounds it to float32
 *   terminated_dev, truncated_dev, status_dev   [K,N] uint8 (0 / 1, 0 / 1, CS_STATUS_*)
 * Each of them may be NULL (not written).  These are bit-identical to an env with auto-reset disabled stepped K times.
 * Start point: start_x_dev == NULL = the stored state the next cs_step starts from: its pending perturbation enters the
 * first call of step 1, and a lane with a NEXT_STEP reset pending performs that reset in step 1 with the draw cs_step
 * would make (that lane's gradient with respect to x0 and the first action is zero).  Or an explicit point:
 * start_x_dev [12,N] float64 + start_status_dev [N] (both required) + optional start_force_dev [3,N] newtons, pending,
 * and optional start_prev_shaping_dev [N] (NaN = upstream's None: reward 0 in step 1).  Without prev_shaping it is
 * shaping(x0), DIFFERENTIATED, so that the telescoping reward holds from step 1; a given prev_shaping is a constant.
 * The step counter (time-limit truncation) is the env's stored one in both cases.
 *
 * cs_rollout_vjp (backward): given cotangents gx_dev [K,N,12] (on x) and gr_dev [K,N] (on reward), float64, either
 * NULL = zero, writes
 *   g_actions_dev  [K,N,A]  dL / d actions, the actions as cs_step receives them (the clip's derivative is 1 on [0, 1],
 *                           0 outside)
 *   g_x0_dev       [12,N]   dL / d x0 (an explicit start's x; with the stored start: the decoded words)
 * in out_dtype (CS_JAC_F64, or CS_JAC_F32: the float64 values rounded); either may be NULL.  The tape is the forward's
 * own output: x_dev and status_dev are READ (both required), with the same K, actions and start point; a stored start
 * is decoded again, so the env must not have been stepped, reset or set in between.  The derivative rules are those of
 * cs_step_jacobian (the float64 motor law's derivative also under action_arith = CS_ARITH_F32; LANDED, ground contact,
 * CRASHED and LEVELING as there; a tilt, a prev_shaping of None and the Hover tasks give no reward gradient; the
 * storage rounding of the float32 modes is the identity), plus the one term a single step cannot see: reward_k depends
 * on x_{k-1} through prev_shaping.  The perturbation force and the vehicle are constants here; cs_rollout_vjp_ex
 * (below) differentiates with respect to them as well.
 *
 * Asynchronous on `stream`.  io->struct_size must be sizeof(cs_rollout_io) (else CS_ERR_ABI); the argument block is
 * checked before the context. */
typedef struct cs_rollout_io {
  uint32_t struct_size;                /* sizeof(cs_rollout_io) */
  uint32_t out_dtype;                  /* CS_JAC_F64 / CS_JAC_F32: g_actions_dev, g_x0_dev */
  int32_t num_steps;                   /* K >= 1 */
  uint32_t reserved_;                  /* 0 */
  const float* actions_dev;            /* [K,N,A] float32, required */
  const double* start_x_dev;           /* [12,N] explicit start, or NULL = the stored state */
  const uint8_t* start_status_dev;     /* [N] required with start_x_dev */
  const double* start_force_dev;       /* [3,N] newtons, optional with start_x_dev */
  const double* start_prev_shaping_dev; /* [N], optional with start_x_dev */
  double* x_dev;                       /* [K,N,12]: written by cs_rollout_states, read by cs_rollout_vjp */
  double* reward_dev;                  /* [K,N] */
  uint8_t* terminated_dev;             /* [K,N] */
  uint8_t* truncated_dev;              /* [K,N] */
  uint8_t* status_dev;                 /* [K,N]: written by cs_rollout_states, read by cs_rollout_vjp */
  const double* gx_dev;                /* [K,N,12] float64 or NULL */
  const double* gr_dev;                /* [K,N] float64 or NULL */
  void* g_actions_dev;                 /* [K,N,A] */
  void* g_x0_dev;                      /* [12,N] */
} cs_rollout_io;
int cs_rollout_states(cs_ctx* ctx, const cs_rollout_io* io, void* stream);
int cs_rollout_vjp(cs_ctx* ctx, const cs_rollout_io* io, void* stream);

/* Rollouts as functions of the vehicle and of the start's pending force: system identification,
 * disturbance estimation, sensitivity to the vehicle.  cs_rollout_states_ex / cs_rollout_vjp_ex take cs_rollout_io as
 * cs_rollout_states / cs_rollout_vjp do, plus
 *   vehicle_dev    [12,N] float64, cs_set_vehicle_params' rows (B, D, M, L, Ix, Iy, Iz, Jr, maxrpm, G, rho, C_L), or
 *                  NULL = the env's own vehicle (its per-env table, else cs_config's).  A table given here is folded on
 *                  the device into a scratch table of the context, bit for bit as cs_set_vehicle_params folds it, and is
 *                  used by THIS call only: the env's installed vehicle is untouched and the rollout stays a pure
 *                  function.  It cannot be checked synchronously: the caller guarantees M, Ix, Iy, Iz > 0 and every
 *                  value finite (cs_set_vehicle_params' contract; gym_copter_amd checks it with a device reduction).  A
 *                  cs_rollout_vjp_ex must be given the same vehicle as the cs_rollout_states_ex that made its tape.
 *   g_vehicle_dev  [12,N] dL / d vehicle, per env (callers sum over envs for a shared vehicle); rows that do not enter
 *                  the configuration are 0: B under CS_THRUST_LIFT, rho and C_L under CS_THRUST_B, Jr without
 *                  rotor_gyro.  Written by cs_rollout_vjp_ex; NULL = not wanted.
 *   g_force_dev    [3,N] dL / d the start's pending force, newtons (an explicit start's start_force_dev, or the stored
 *                  start's pending perturbation).  Exactly 0 where no perturbation is pending (the stored start's was
 *                  consumed, or an explicit start has no start_force_dev: pass a zero start_force_dev for the
 *                  sensitivity at F = 0), where it never integrates (kept pending by a ground-contact freeze), and for
 *                  a lane with a NEXT_STEP reset pending: the new episode's draw is a constant (the steps after that
 *                  reset still contribute to g_vehicle).  Written by cs_rollout_vjp_ex; NULL = not wanted.
 * g_vehicle_dev and g_force_dev are in out_dtype (CS_JAC_F64 or CS_JAC_F32); cs_rollout_states_ex reads vehicle_dev
 * only.  The storage rounding is the identity, as in cs_rollout_vjp.  With pio == NULL both calls are exactly
 * cs_rollout_states / cs_rollout_vjp.  Refused (CS_ERR_ARG) under action_arith = CS_ARITH_F32.  The first call with a
 * vehicle_dev or a gradient allocates the context's scratch tables (call it outside graph capture); calls on one context
 * that use them must be ordered on one stream. */
typedef struct cs_rollout_param_io {
  uint32_t struct_size;        /* sizeof(cs_rollout_param_io) */
  uint32_t out_dtype;          /* CS_JAC_F64 / CS_JAC_F32: g_vehicle_dev, g_force_dev */
  const double* vehicle_dev;   /* [12,N] float64 raw vehicle for this call, or NULL */
  void* g_vehicle_dev;         /* [12,N] */
  void* g_force_dev;           /* [3,N] newtons */
} cs_rollout_param_io;
int cs_rollout_states_ex(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_param_io* pio, void* stream);
int cs_rollout_vjp_ex(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_param_io* pio, void* stream);

/* Forward-mode tangents of a rollout (the lines differentiated are cs_rollout_vjp's:
 * dynamics/__init__.py:114-197, :249-302; envs/task.py:77-137; envs/lander.py:46-74).  Where cs_rollout_vjp /
 * cs_rollout_vjp_ex pull ONE cotangent back through the K steps, cs_jvp_rollout pushes D input directions forward: the
 * shape for problems with a handful of inputs and K x 12 outputs (system identification by Gauss-Newton, disturbance
 * estimation, the sensitivity of a plan to the vehicle, Gauss-Newton Hessian-vector products J^T (J v)).
 *   t_actions_dev  [D,K,N,A] float64  tangent of the actions as cs_step receives them (the clip's derivative is 1 on
 *                                     [0, 1], 0 outside), or NULL = zero
 *   t_x0_dev       [D,12,N]  float64  tangent of the start state (an explicit start's x; with the stored start: the
 *                                     decoded words), or NULL
 *   t_vehicle_dev  [D,12,N]  float64  tangents of the raw rows of cs_set_vehicle_params (B, D, M, L, Ix, Iy, Iz, Jr,
 *                                     maxrpm, G, rho, C_L), or NULL
 *   t_force_dev    [D,3,N]   float64  newtons: tangent of the start's pending force (an explicit start's
 *                                     start_force_dev, or the stored start's pending perturbation), or NULL
 *   vehicle_dev    [12,N]             the vehicle of THIS call, exactly as cs_rollout_param_io's: the one that the
 *                                     cs_rollout_states_ex that made the tape was given, or NULL = the env's own
 *   t_x_dev        [D,K,N,12] out     tangent of x_dev row k;  t_reward_dev [D,K,N] out: tangent of reward_dev
 * in out_dtype (CS_JAC_F64, or CS_JAC_F32: the float64 values rounded).  At least one input tangent and at least one
 * output must be given; t_x_dev must be 16-byte aligned.  1 <= num_dirs <= CS_JVP_MAX_DIRS.
 *
 * io is used as cs_rollout_vjp uses it -- the same K, actions and start point; io->x_dev and io->status_dev are the
 * forward's tape, READ, both required; a stored start is decoded again, so the env must not have been stepped, reset or
 * set in between -- except that io's reward_dev, terminated_dev, truncated_dev, gx_dev, gr_dev, g_actions_dev and
 * g_x0_dev must be NULL.  Every refusal is CS_ERR_ARG (CS_ERR_ABI for a wrong struct_size), its message starts with
 * "cs_jvp_rollout:" and names the member; the blocks are checked before the context.
 *
 * The linear map is exactly the one whose transpose cs_rollout_vjp and cs_rollout_vjp_ex apply, at the tape's points:
 * for every env, <gx, t_x> + <gr, t_reward> = <g_actions, t_actions> + <g_x0, t_x0> + <g_vehicle, t_vehicle> +
 * <g_force, t_force>.  The storage rounding of the float32 modes is straight-through.  LANDED (task.py:86-87), ground
 * contact, LEVELING (dynamics/__init__.py:174-175) and CRASHED rows behave as in cs_step_jacobian.  A lane with a
 * NEXT_STEP reset pending at a stored start has its x0, first-action and force tangents zeroed by that reset; the steps
 * after it still carry the vehicle tangent, including d(2 / M) times the new episode's draw.  The force tangent is
 * exactly 0 where no force is pending (consumed, or an explicit start without start_force_dev) and where the force
 * never integrates.  Vehicle rows that do not enter the configuration contribute exactly 0: B under CS_THRUST_LIFT, rho
 * and C_L under CS_THRUST_B, Jr without rotor_gyro.  The reward tangent of step k is grad shaping(x_k) . t_x_k minus
 * grad shaping(x_{k-1}) . t_x_{k-1} wherever the backward differentiates prev_shaping (lander.py:59-62; every step but
 * the first, and the first of an explicit start without start_prev_shaping_dev); it is zero where the backward gives
 * no reward gradient: a tilt, a prev_shaping of None, a reset, and the Hover tasks.
 *
 * With t_vehicle_dev, t_force_dev or vehicle_dev the call is refused under action_arith = CS_ARITH_F32, as
 * cs_rollout_vjp_ex is; the plain tangents use the float64 motor law's derivative there, as cs_rollout_vjp does.  A
 * vehicle_dev uses the context's scratch table as cs_rollout_states_ex does (first use allocates: outside graph
 * capture; such calls on one context are ordered on one stream).  Nothing of the env is written.  Asynchronous on
 * `stream`. */
#define CS_JVP_MAX_DIRS 64
typedef struct cs_jvp_io {
  uint32_t struct_size;          /* sizeof(cs_jvp_io) */
  uint32_t out_dtype;            /* CS_JAC_F64 / CS_JAC_F32: t_x_dev, t_reward_dev */
  int32_t num_dirs;              /* D: 1 .. CS_JVP_MAX_DIRS */
  uint32_t reserved_;            /* 0 */
  const double* t_actions_dev;   /* [D,K,N,A] or NULL */
  const double* t_x0_dev;        /* [D,12,N] or NULL */
  const double* t_vehicle_dev;   /* [D,12,N] or NULL */
  const double* t_force_dev;     /* [D,3,N] newtons, or NULL */
  const double* vehicle_dev;     /* [12,N] float64 raw vehicle for this call, or NULL */
  void* t_x_dev;                 /* [D,K,N,12] */
  void* t_reward_dev;            /* [D,K,N] */
} cs_jvp_io;
int cs_jvp_rollout(cs_ctx* ctx, const cs_rollout_io* io, const cs_jvp_io* jio, void* stream);

/* Differentiable CLOSED-LOOP rollouts under a fused MLP policy: analytic policy gradients
 * (backpropagation through the simulator) without a Python loop.  The loop replaced is lander.py:40-65 with a policy in
 * place of the random action -- observe, act, step -- K times.  A closed-loop rollout is K calls of cs_step with auto-reset
 * disabled in which step k = 1..K takes
 *     a_k = fl32( pi_theta(o_{k-1}) + u_k )
 * o_{k-1} is the float32 observation cs_step returns for the state before step k (the task's obs_dim state slots from
 * its first observed slot: what a copterstep_rollout.h policy receives; for k = 1 that of the start point, stored or
 * explicit); u_k = offsets_dev[k-1] (NULL = 0).  Everything else -- the start point, the pending perturbation, a
 * NEXT_STEP reset pending at the start, prev_shaping, the step counter, no env state written -- is cs_rollout_states'.
 *
 * The policy is an MLP shared by every env, one flat float32 parameter vector theta = params_dev:
 *   hidden = 0:        a = W o + b                          [W (A x OBS, row-major), b (A)]            P = A (OBS + 1)
 *   1 <= hidden <= 64: h = tanh(W1 o + b1), a = W2 h + b2   [W1 (H x OBS), b1 (H), W2 (A x H), b2 (A)]
 *                                                           P = H (OBS + 1) + A (H + 1)
 * Its float32 arithmetic is fixed (no dependence on the compiler's contraction): every sum is an fmaf chain that starts
 * from its bias and adds the terms in index order -- pre_j = fmaf(W1[j][OBS-1], o[OBS-1], ... fmaf(W1[j][0], o[0], b1[j])),
 * h_j = tanhf(pre_j) (the device library's tanhf), a_c = fmaf(W2[c][H-1], h_{H-1}, ... fmaf(W2[c][0], h_0, b2[c])) --
 * and a_k = a + u_k is one float32 addition (skipped when offsets_dev is NULL).
 *
 * cs_rollout_mlp_states (forward) writes cs_rollout_io's x, reward, flag and status outputs as cs_rollout_states does
 * (bit-identical to an env with auto-reset disabled stepped with actions_out_dev), plus
 *   actions_out_dev  [K,N,A] float32  a_k (required: it is the backward's tape)
 *   obs_out_dev      [K,N,OBS] float32 o_{k-1}, or NULL (not written)
 * cs_rollout_mlp_vjp (backward) reads the tape (io x_dev, status_dev and actions_out_dev, the forward's own, with the
 * same params, hidden and start; offsets_dev and obs_out_dev are not read) and writes, in io->out_dtype,
 *   g_actions_dev    [K,N,A]  dL / d a_k INCLUDING every later step's dependence on a_k through the policy; = dL / d u_k
 *   g_x0_dev         [12,N]   dL / d x0 (an explicit start), including the path through o_0
 * The derivative rules are cs_rollout_vjp's plus the policy's: the float32 rounding of o and of a is straight-through
 * (as the storage rounding is), tanh' = 1 - h^2 with h recomputed in float64, lambda_o += J_o pi^T g_a accumulated in
 * float64.  A lane that resets in step 1 has g_a_1 = 0, so the policy adds nothing through a_1.  The gradient with
 * respect to theta is a reduction over every env and step of the obs tape and g_actions:
 *     g_theta = sum_{k,n} J_theta pi(o_{k-1,n})^T g_a_{k,n}
 * (cs_mlp_param_grad below, on the device; gym_copter_amd.mlp.param_grad is the same sum as torch matrix products: h
 * recomputed in float64, as the kernel does).
 *
 * io->actions_dev must be NULL in both calls (the policy makes the actions).  params_dev is read by the scalar unit:
 * 4-B aligned, never written while a call runs; actions_out_dev and obs_out_dev 16-B aligned.  The vehicle override and
 * parameter gradients of cs_rollout_param_io are not part of these calls.  Asynchronous on `stream`;
 * mio->struct_size must be sizeof(cs_rollout_mlp_io) (else CS_ERR_ABI); both blocks are checked before the context. */
#define CS_MLP_MAX_HIDDEN 64
typedef struct cs_rollout_mlp_io {
  uint32_t struct_size;        /* sizeof(cs_rollout_mlp_io) */
  int32_t hidden;              /* 0 .. CS_MLP_MAX_HIDDEN */
  const float* params_dev;     /* [P] float32, required */
  const float* offsets_dev;    /* [K,N,A] u, or NULL */
  float* actions_out_dev;      /* [K,N,A] a_k: written by _states, read by _vjp as the tape (required) */
  float* obs_out_dev;          /* [K,N,OBS] o_{k-1}: written by _states, NULL = not written */
} cs_rollout_mlp_io;
int cs_rollout_mlp_states(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_mlp_io* mio, void* stream);
int cs_rollout_mlp_vjp(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_mlp_io* mio, void* stream);

/* cs_rollout_mlp_vjp with a cotangent on the ACTION TAPE: a loss that depends on the actions themselves (control effort,
 * action rate).  xio->g_actions_in_dev [K,N,A] float64 (NULL = zero) is the caller's dL / d a_k taken directly on
 * actions_out_dev.  a_k is the action as cs_step receives it, before the clip, so the cotangent adds without a mask:
 *     g_a_k = (the step's own adjoint of a_k) + g_actions_in[k]
 * and that total is what g_actions_dev receives and what the policy's vector-Jacobian product pushes into the state's
 * adjoint; g_actions_dev is still dL / d u_k and still the input of the theta reduction below.  A lane that resets in
 * step 1 (a stored start with a NEXT_STEP reset pending) gets g_actions[0] = g_actions_in[0], and its policy product
 * stays skipped (its pre-reset state need not be finite, and a stored start returns no g_x0).  With xio == NULL, or a
 * NULL g_actions_in_dev, the call is exactly cs_rollout_mlp_vjp.  xio->struct_size must be
 * sizeof(cs_rollout_mlp_ex_io) (else CS_ERR_ABI); the blocks are checked before the context. */
typedef struct cs_rollout_mlp_ex_io {
  uint32_t struct_size;            /* sizeof(cs_rollout_mlp_ex_io) */
  uint32_t reserved_;              /* 0 */
  const double* g_actions_in_dev;  /* [K,N,A] float64 dL / d a_k on the action tape, or NULL = zero */
} cs_rollout_mlp_ex_io;
int cs_rollout_mlp_vjp_ex(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_mlp_io* mio,
                          const cs_rollout_mlp_ex_io* xio, void* stream);

/* The gradient with respect to theta, on the device: g_params = sum_{k,n} J_theta pi(o_{k-1,n})^T g_a_{k,n} over the
 * forward's obs tape and the backward's g_actions (N, OBS and A are the context's).  Per row, in float64:
 *   o = (double)obs;  pre_j = fma chain from (double)b1[j] in index order;  h_j = tanh(pre_j) (the device library's
 *   float64 tanh: what cs_rollout_mlp_vjp recomputes);  gh_j = sum_c W2[c][j] g_a[c];  gp_j = gh_j (1 - h_j^2);
 *   gW1[j][i] += gp_j o_i;  gb1[j] += gp_j;  gW2[c][j] += g_a[c] h_j;  gb2[c] += g_a[c]
 * (hidden = 0: gW[c][i] += g_a[c] o_i, gb[c] += g_a[c]) -- gym_copter_amd.mlp.param_grad term by term.  The order of
 * summation is the kernel's own and fixed (a function of K N and the shape; no floating-point atomics): the same inputs
 * give the same bits on every call.  g_params_dev is WRITTEN, not accumulated.  Asynchronous on `stream`; obs_dev and
 * g_actions_dev are aligned to their element size.  The first call on a context allocates its scratch of partial sums
 * (call it outside graph capture; released by cs_destroy), and calls on one context must be ordered on one stream.
 * io->struct_size must be sizeof(cs_mlp_grad_io) (else CS_ERR_ABI); the block is checked before the context. */
typedef struct cs_mlp_grad_io {
  uint32_t struct_size;        /* sizeof(cs_mlp_grad_io) */
  uint32_t ga_dtype;           /* CS_JAC_F64 / CS_JAC_F32: the dtype of g_actions_dev */
  int32_t hidden;              /* 0 .. CS_MLP_MAX_HIDDEN */
  int32_t num_steps;           /* K >= 1 */
  const float* params_dev;     /* [P] float32, cs_rollout_mlp_io's layout */
  const float* obs_dev;        /* [K,N,OBS] float32: the forward's obs tape */
  const void* g_actions_dev;   /* [K,N,A]: what cs_rollout_mlp_vjp wrote */
  double* g_params_dev;        /* [P] float64: WRITTEN, not accumulated */
} cs_mlp_grad_io;
int cs_mlp_param_grad(cs_ctx* ctx, const cs_mlp_grad_io* io, void* stream);

/* The iLQR backward pass over a rollout's tape, on the device: a second-order trajectory
 * optimiser's Riccati sweep without the K dense Jacobian blocks.  The caller's cost is J = sum_{k=1..K} [l_k(x_k) +
 * m_k(a_k)], given by its quadratic model at the tape:
 *   q_dev       [K,N,12] float64  grad l_k at x_k (row k-1), NULL = zero
 *   r_dev       [K,N,A]  float64  grad m_k at a_k (row k-1), NULL = zero
 *   Q_dev       [12,12]  float64  the Hessian of l_k, symmetric PSD, shared by every env and step (required)
 *   Q_final_dev [12,12]           replaces Q_dev at k = K, or NULL
 *   R_dev       [A,A]    float64  the Hessian of m_k, symmetric PD, shared (required)
 *   mu          >= 0              the Levenberg term
 * (Gauss-Newton: no second derivatives of the dynamics enter).  With A_k = d x_k / d x_{k-1} and B_k = d x_k / d a_k --
 * cs_step_jacobian's dx and du at (tape row k-2, its status, action k), every rule of that call included (the clip's
 * zero columns, the identity of LANDED / contact / CRASHED, LEVELING's zero rows, A = B = 0 for a NEXT_STEP reset in
 * step 1, straight-through storage rounding, the float64 motor law's derivative also under CS_ARITH_F32, the pending
 * perturbation of step 1 and the redraw of step 2 after a reset as cs_rollout_vjp recomputes them); never written to
 * memory -- the call runs, in float64, from S = 0, s = 0 beyond the horizon, for k = K .. 1:
 *   V = S + Q_k,  v = s + q_k
 *   Qx = A^T v,  Qu = r_k + B^T v,  Qxx = A^T V A,  Qux = B^T V A,  Quu = R + B^T V B
 *   K_k = -(Quu + mu I)^-1 Qux,  d_k = -(Quu + mu I)^-1 Qu        (a Cholesky factorisation of the A x A matrix)
 *   S <- Qxx + K^T Quu K + K^T Qux + Qux^T K  (its upper triangle kept),  s <- Qx + K^T Quu d + K^T Qu + Qux^T d
 *   dV1 += d^T Qu,  dV2 += 1/2 d^T Quu d
 * so that the model's prediction of the cost change under a_k + alpha d_k + K_k (x_{k-1} - xbar_{k-1}) is
 * alpha dV1 + alpha^2 dV2.  Outputs, each may be NULL, in lio->out_dtype (CS_JAC_F64, or CS_JAC_F32: the float64 values
 * rounded):
 *   K_dev  [K,N,A,12]   d_dev  [K,N,A]   dV_dev [N,2]   S0_dev [N,12,12] and s0_dev [12,N]: S and s at the start
 *   ok_dev [N] uint8    0 if any Cholesky pivot of the env was <= 0 or not finite (its gains are still written, finite
 *                       or not: raise mu), else 1
 * io is cs_rollout_vjp's block -- the tape x_dev / status_dev, actions_dev, num_steps and the start point of the
 * cs_rollout_states call that made the tape; its cotangents and gradient outputs are not used.  Nothing of the env
 * state is written.  Asynchronous on `stream`; lio->struct_size must be sizeof(cs_rollout_lqr_io) (else CS_ERR_ABI);
 * both blocks are checked before the context.  The shared matrices are read by the scalar unit: 8-B aligned, never
 * written while a call runs. */
typedef struct cs_rollout_lqr_io {
  uint32_t struct_size;        /* sizeof(cs_rollout_lqr_io) */
  uint32_t out_dtype;          /* CS_JAC_F64 / CS_JAC_F32: K_dev, d_dev, dV_dev, S0_dev, s0_dev */
  double mu;                   /* >= 0, finite */
  const double* q_dev;         /* [K,N,12] or NULL */
  const double* r_dev;         /* [K,N,A] or NULL */
  const double* Q_dev;         /* [12,12], required */
  const double* Q_final_dev;   /* [12,12] or NULL */
  const double* R_dev;         /* [A,A], required */
  void* K_dev;                 /* [K,N,A,12] */
  void* d_dev;                 /* [K,N,A] */
  void* dV_dev;                /* [N,2] */
  void* S0_dev;                /* [N,12,12] */
  void* s0_dev;                /* [12,N] */
  uint8_t* ok_dev;             /* [N] */
} cs_rollout_lqr_io;
int cs_rollout_lqr(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_lqr_io* lio, void* stream);

/* The iLQR forward pass (line search): cs_rollout_states with a time-varying affine feedback as its action source.
 * Step k = 1..K takes
 *     a_k = fl32( abar_k + alpha d_k + K_k (x_{k-1} - xbar_{k-1}) )
 * x_{k-1} is the decoded stored state of THIS rollout before step k; xbar the nominal tape (xbar_dev row k-2; xbar_0 is
 * the shared start point, so step 1 has no deviation term); abar = io->actions_dev, the nominal actions; alpha per env.
 * The arithmetic is fixed, float64 without contraction: t = abar + alpha d (one multiply, one add); then for j = 0..11
 * in order t += K[c][j] (x[j] - xbar[j]) (a subtraction, a multiply, an add); one rounding to float32.  Outputs are
 * cs_rollout_states' (io's x, reward, flags, status; bit-identical to cs_rollout_states fed actions_out_dev) plus
 *   actions_out_dev [K,N,A] float32  a_k (required)
 * Everything else -- the start point, the pending perturbation, a pending NEXT_STEP reset, prev_shaping, the step
 * counter, no env state written -- is cs_rollout_states'.  K_dev and d_dev are float64 (cs_rollout_lqr's with
 * CS_JAC_F64).  fio->struct_size must be sizeof(cs_rollout_feedback_io) (else CS_ERR_ABI). */
typedef struct cs_rollout_feedback_io {
  uint32_t struct_size;        /* sizeof(cs_rollout_feedback_io) */
  uint32_t reserved_;          /* 0 */
  const double* xbar_dev;      /* [K,N,12] the nominal tape (rows 0 .. K-2 are read; may be NULL when K = 1) */
  const double* K_dev;         /* [K,N,A,12] float64, required */
  const double* d_dev;         /* [K,N,A] float64, required */
  const double* alpha_dev;     /* [N] float64, required */
  float* actions_out_dev;      /* [K,N,A] float32, required */
} cs_rollout_feedback_io;
int cs_rollout_feedback_states(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_feedback_io* fio, void* stream);

/* Control-limited iLQR (Tassa, Mansard, Todorov 2014): the two calls above with the box
 * lo <= a <= hi on the actions handled inside them.  bio carries the box and the calls' extra outputs; io, lio and fio
 * are the blocks of cs_rollout_lqr and cs_rollout_feedback_states, unchanged.  Every block is checked before the
 * context, bio last; bio->struct_size must be sizeof(cs_ilqr_box_io) (else CS_ERR_ABI).
 *
 * cs_ilqr_box_backward is cs_rollout_lqr in every respect but the solve of a step.  With H = Quu + mu I, g = Qu and
 * abar the step's nominal action widened to float64, l = lo - abar and u = hi - abar (one subtraction each), d_k
 * minimises 1/2 d^T H d + g^T d over l <= d <= u by projected Newton steps whose arithmetic is fixed
 * (gym_copter_amd/csrc/boxqp_solve.h states it; tests/boxqp_ref.py restates it):
 *   start      x = clamp(-(H^-1 g)) with cs_rollout_lqr's Cholesky factor of H
 *   iteration  gr = g + Hx; control a is clamped if (x_a <= l_a and gr_a > 0) or (x_a >= u_a and gr_a < 0), else free;
 *              none free: stop.  The free block is solved with the same Cholesky on the masked matrix (H_ab where both
 *              are free, delta_ab otherwise; right-hand side -(g_a + sum_{b clamped} H_ab x_b) on free rows, 0 on
 *              clamped ones); s = that solution - x on free rows, 0 elsewhere; max|s| <= 1e-14 max(1, max|x|): stop;
 *              Armijo backtracking x_c = clamp(x + t s), accepted when f(x_c) - f(x) <= 0.1 t gr^T s, else t <- 0.6 t,
 *              at most 30 trials
 *   cap        16 iterations.  An env that exhausts them (or an iteration none of whose trials is accepted), or whose
 *              masked factor has a pivot <= 0 or not finite, gets ok = 0; its outputs are written regardless.
 * d_k = x; the free rows of K_k are -(H_ff)^-1 Qux_f (the masked factor, the masked right-hand side, column by column),
 * its clamped rows are 0.  S, s, dV1 += d^T Qu and dV2 += 1/2 d^T Quu d (the unregularised Quu) are cs_rollout_lqr's
 * expressions at these K, d.  The first step of a lane with a NEXT_STEP reset pending (the env ignores its action:
 * Qux = 0, Quu = R) takes the start, clamped, and no iteration.  With lo = -inf and hi = +inf every output equals
 * cs_rollout_lqr's bit for bit.
 *
 * cs_ilqr_box_forward is cs_rollout_feedback_states with one more operation after the rounding to float32:
 * a = a < lo ? lo : (a > hi ? hi : a) in float32 (a NaN stays a NaN).  The clamped value is what actions_out_dev
 * receives and what the step takes; the outputs are bit-identical to cs_rollout_states fed actions_out_dev. */
typedef struct cs_ilqr_box_io {
  uint32_t struct_size;        /* sizeof(cs_ilqr_box_io) */
  uint32_t reserved_;          /* 0 */
  const float* lo_dev;         /* [A] float32, required; -inf allowed */
  const float* hi_dev;         /* [A] float32, required; +inf allowed; lo <= hi is the caller's to guarantee */
  uint8_t* clamped_dev;        /* [K,N] or NULL.  backward: bit a = control a held at its lower bound, bit 4+a = at its
                                  upper (the set of the last iteration).  forward: the same bits for where the clamp
                                  changed the action */
  uint8_t* iters_dev;          /* [K,N] or NULL, backward only (forward: must be NULL): iterations used, 0 on a
                                  resetting lane's step 1 */
} cs_ilqr_box_io;
int cs_ilqr_box_backward(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_lqr_io* lio, const cs_ilqr_box_io* bio,
                         void* stream);
int cs_ilqr_box_forward(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_feedback_io* fio,
                        const cs_ilqr_box_io* bio, void* stream);

/* An extended Kalman filter over the env step, on the device: K predict / update steps per env
 * in one call, the step Jacobian applied on the fly and never stored.  The filter's state -- the mean xhat [12] and the
 * covariance P [12,12] -- is the CALLER's: no env state is read except the context's constants and vehicle table, and
 * none is written.  The measurement model is linear and shared, z = H x + e with e ~ N(0, diag(r)); the process noise Q
 * is additive per step.
 *
 * From io: num_steps = K, actions_dev [K,N,A], start_x_dev [12,N] = xhat_0 and start_status_dev [N] (both required);
 * start_force_dev and start_prev_shaping_dev must be NULL (no perturbation is pending: disturbances are what Q models);
 * x_dev [K,N,12] (or NULL) receives the filtered means and status_dev [K,N] (or NULL) the flight status the filter's own
 * mean has after step k; the reward, flag, cotangent and gradient pointers must be NULL.
 *
 * From eio:
 *   num_meas  M, 1 .. CS_EKF_MAX_MEAS
 *   H_dev     [M,12]    float64  shared by all envs and steps
 *   r_dev     [M]       float64  the measurement variances, each finite and > 0 (the caller's to guarantee;
 *                                gym_copter_amd checks them)
 *   Q_dev     [12,12]   float64  symmetric PSD, shared
 *   P0_dev    [N,12,12] float64  symmetric: its upper triangle is read
 *   z_dev     [K,N,M]   float64  a NaN entry means "no measurement": that scalar update is skipped
 * Per step k = 1..K and env, in float64 without contraction:
 *   predict   x- = the physics of step k from (xhat, status) under actions[k-1], as cs_rollout_states takes it from that
 *             explicit point (clip, fan-out, the env's vehicle, the thrust law, the gyro term, `substeps` calls, the
 *             status machine), without storage rounding; termination and auto-reset do not enter.
 *             P- = A P A^T + Q with A = cs_step_jacobian's dx at that point under every rule of that call (LANDED:
 *             identity; contact and CRASHED calls hold; LEVELING zeroes the phi, theta rows); CS_JAC_RESET never
 *             occurs.  The upper triangle is kept; one add per entry applies Q.
 *   update    for i = 0 .. M-1 in order, skipping NaN z_i:  h = H[i],  p = P h,  s = h^T p + r_i,  nu = z_i - h^T x,
 *             g = p / s,  x <- x + g nu,  P <- P - g p^T (upper triangle),  nis += nu^2 / s,
 *             loglik -= 1/2 (nu^2 / s + ln(2 pi s)).  Sequential scalar updates are exact for a diagonal R, and the sum
 *             of nu^2 / s over a step is its joint normalised innovation squared.  If s is not finite or <= 0 the
 *             env's ok is 0; every output is written regardless.
 * Outputs, each may be NULL; P, P_tape, var, nis and loglik in out_dtype (CS_JAC_F64, or CS_JAC_F32: the float64 values
 * rounded):
 *   x_pred_dev [K,N,12] float64  the prior means x-          P_dev      [N,12,12]   the posterior after step K (full,
 *   P_tape_dev [K,N,12,12]       the posterior of every step                          symmetric)
 *   var_dev    [K,N,12]          the posterior's diagonal    nis_dev    [K,N]       the step's sum of nu^2 / s
 *   loglik_dev [N]               the call's log-likelihood   branch_dev [K,N] uint8 the CS_JAC_* bits of the step
 *   ok_dev     [N] uint8
 * Refused (CS_ERR_ARG) under action_arith = CS_ARITH_F32.  Asynchronous on `stream`; eio->struct_size must be
 * sizeof(cs_rollout_ekf_io) (else CS_ERR_ABI); both blocks are checked before the context.  H, r and Q are read by the
 * scalar unit: 8-B aligned (as every float64 array here), never written while a call runs. */
#define CS_EKF_MAX_MEAS 12
typedef struct cs_rollout_ekf_io {
  uint32_t struct_size;        /* sizeof(cs_rollout_ekf_io) */
  uint32_t out_dtype;          /* CS_JAC_F64 / CS_JAC_F32: P_dev, P_tape_dev, var_dev, nis_dev, loglik_dev */
  int32_t num_meas;            /* M, 1 .. CS_EKF_MAX_MEAS */
  uint32_t reserved_;          /* 0 */
  const double* H_dev;         /* [M,12], required */
  const double* r_dev;         /* [M], required */
  const double* Q_dev;         /* [12,12], required */
  const double* P0_dev;        /* [N,12,12], required */
  const double* z_dev;         /* [K,N,M], required */
  double* x_pred_dev;          /* [K,N,12] */
  void* P_dev;                 /* [N,12,12] */
  void* P_tape_dev;            /* [K,N,12,12] */
  void* var_dev;               /* [K,N,12] */
  void* nis_dev;               /* [K,N] */
  void* loglik_dev;            /* [N] */
  uint8_t* branch_dev;         /* [K,N] */
  uint8_t* ok_dev;             /* [N] */
} cs_rollout_ekf_io;
int cs_rollout_ekf(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_ekf_io* eio, void* stream);

/* A Rauch-Tung-Striebel fixed-interval smoother over the tapes of cs_rollout_ekf, on the device:
 * the estimate of every step given the measurements of all K steps, in one call of K backward steps per env.  The step
 * Jacobian is applied on the fly, at the filter's own points, and never stored.  No env state is read except the
 * context's constants and vehicle table, and none is written.
 *
 * Row k = 0 .. K-1 of a tape is the state after step k+1; "row -1" is the filter's starting point (x0, P0, status0).
 *
 * From io: num_steps = K, actions_dev [K,N,A] (the filter's), start_x_dev [12,N] = x0 and start_status_dev [N] = status0
 * (both required); x_dev [K,N,12] (or NULL) receives the smoothed means; every other pointer of io must be NULL.
 *
 * From rio, the inputs (float64; the four tapes are cs_rollout_ekf's x_dev, x_pred_dev, status_dev and, with CS_JAC_F64,
 * P_tape_dev of the call that filtered these K steps from this starting point with this Q):
 *   x_f_dev      [K,N,12]     the filtered means        x_pred_dev [K,N,12]  the prior means
 *   status_f_dev [K,N] uint8  the filter's status       P_f_dev    [K,N,12,12]  the posteriors: upper triangles are read
 *   Q_dev        [12,12]      symmetric positive definite, shared (a merely PSD Q can make a prior singular: ok = 0)
 *   P0_dev       [N,12,12]    symmetric: its upper triangle is read
 *   end_x_dev [12,N], end_P_dev [N,12,12]   both or neither (NULL): the smoothed row K-1, for a caller that smooths a
 *                             long tape in chunks, last chunk first: the smoothed starting point of the following chunk
 * The smoothed row K-1 is given: the filter's own row K-1, or (end_x, the upper triangle of end_P, mirrored); it is
 * written out as it is.  Then for j = K-2 down to -1 and every env, in float64 without contraction:
 *   predict   A = cs_step_jacobian's dx at (x_f[j], status_f[j]) under actions[j+1], with every rule of that call and a
 *             zero wrench tangent: the point and the wrench cs_rollout_ekf used for step j+2.  W = A P_f[j];
 *             P- = W A^T + Q, the upper triangle kept, one add per entry for Q: the filter's own prior, bit for bit.
 *   solve     P- = L L^T by Cholesky.  If a pivot is <= 0 or not finite the env's ok is 0; the arithmetic is carried
 *             through and every output is written regardless.  G = P-^-1 W by a forward and a backward substitution per
 *             column (the smoother gain is G^T).
 *   smooth    x_s[j] = x_f[j] + G^T (x_s[j+1] - x_pred[j+1]);  P_s[j] = P_f[j] + G^T (P_s[j+1] - P-) G, its upper
 *             triangle computed and mirrored on store.
 * The order of every sum is fixed (gym_copter_amd/csrc/rts_solve.h).
 * Outputs, each may be NULL; P_tape, var and P0_s in out_dtype (CS_JAC_F64, or CS_JAC_F32: the float64 values rounded):
 *   io->x_dev  [K,N,12] float64  the smoothed means           P_tape_dev [K,N,12,12]  the smoothed covariances
 *   var_dev    [K,N,12]          their diagonals              x0_dev     [12,N] float64  the smoothed starting point
 *   P0_s_dev   [N,12,12]         its covariance               ok_dev     [N] uint8
 * No output may overlap an input.  Refused (CS_ERR_ARG) under action_arith = CS_ARITH_F32.  Asynchronous on `stream`;
 * rio->struct_size must be sizeof(cs_rollout_rts_io) (else CS_ERR_ABI); both blocks are checked before the context.  Q
 * is read by the scalar unit: 8-B aligned (as every float64 array here), never written while a call runs. */
typedef struct cs_rollout_rts_io {
  uint32_t struct_size;        /* sizeof(cs_rollout_rts_io) */
  uint32_t out_dtype;          /* CS_JAC_F64 / CS_JAC_F32: P_tape_dev, var_dev, P0_s_dev */
  const double* x_f_dev;       /* [K,N,12], required */
  const double* x_pred_dev;    /* [K,N,12], required */
  const uint8_t* status_f_dev; /* [K,N], required */
  const double* P_f_dev;       /* [K,N,12,12], required */
  const double* Q_dev;         /* [12,12], required */
  const double* P0_dev;        /* [N,12,12], required */
  const double* end_x_dev;     /* [12,N] or NULL */
  const double* end_P_dev;     /* [N,12,12] or NULL (with end_x_dev: both or neither) */
  void* P_tape_dev;            /* [K,N,12,12] */
  void* var_dev;               /* [K,N,12] */
  double* x0_dev;              /* [12,N] */
  void* P0_s_dev;              /* [N,12,12] */
  uint8_t* ok_dev;             /* [N] */
} cs_rollout_rts_io;
int cs_rollout_rts(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_rts_io* rio, void* stream);

/* A bootstrap particle filter over the env step, on the device: K steps of propagate / weight /
 * estimate / resample per env in one call, P particles per env that never leave the compute unit.  The sampling twin of
 * cs_rollout_ekf: a belief that straddles a branch of the step (touchdown, crash, the motor clip) is represented by
 * particles on both sides of it.  The filter's state is the CALLER's: no env state is read except the context's
 * constants and vehicle table, and none is written.  The measurement model is cs_rollout_ekf's, z = H x + e with
 * e ~ N(0, diag(r)); the process noise is additive, w = Lq eps with Lq [12,12] lower triangular (Lq Lq^T = Q; rows of
 * zeros allowed) and shared.  Everything is float64 without contraction unless stated.
 *
 * P = num_particles is a power of two in 64 .. CS_PF_MAX_PARTICLES.  From io: num_steps = K, actions_dev [K,N,A]; the
 * reward, flag, cotangent and gradient pointers, start_force_dev and start_prev_shaping_dev must be NULL.
 *
 * Start, one of two forms (both or neither is refused):
 *   Gaussian  io->start_x_dev [12,N] = xhat_0, io->start_status_dev [N], L0_dev [N,12,12] lower triangular (NULL: every
 *             particle is xhat_0): particle p = xhat_0 + L0 eps(k = 0, p), status = start_status, lw = -ln P
 *   carried   part_in_dev [N,P,12], pstatus_in_dev [N,P], lw_in_dev [N,P] (io->start_x_dev, io->start_status_dev and
 *             L0_dev NULL): what a previous call's part_out_dev, pstatus_out_dev and lw_out_dev hold.  An env's inputs
 *             are read before any of its outputs is written, so the three may be the same buffers as the outputs.
 * first_step >= 1 is the global index of the call's first step: a run in chunks draws what a single call draws.
 *
 * Noise (pf_noise.h).  eps of (seed, global env id g, nonce, step k, particle p, slot j) is one Philox2x32-10 call with
 * counter = (g, nonce) and key = key_pf + ((k * 1024 + p) * 16 + j) mod 2^32, key_pf = the low half of the fifth
 * splitmix64 of the seed; slots 0 .. 11 are the state components (the Irwin-Hall draw of cs_rollout_mppi: float32, mean
 * 0, variance 1 - 2^-32, support +-3.46), slot 12 at p = 0 is the step's resampling word.  noise_i = sum_{j <= i}
 * Lq[i][j] (double)eps_j, j ascending, one multiply and one add per term.  A pure function of its arguments: it does not
 * depend on P, the batch, the sharding or the chunking.
 *
 * Per step k = first_step .. first_step + K - 1 and env:
 *   propagate  every particle goes through the physics of the step from its own (x, status) under the step's action,
 *              exactly as cs_rollout_ekf's mean does (clip, motor law, the env's vehicle, `substeps` calls, the status
 *              machine, skipped for a LANDED particle; no storage rounding, no pending perturbation); then x += noise
 *              for EVERY particle whatever its status -- as cs_rollout_ekf adds Q whatever the branch: Q models what
 *              the step does not, and a caller who wants a landed vehicle to stay put zeroes the rows of Lq it needs.
 *   weight     for the present (not NaN) z_i in order: nu = z_i - H[i] x, ll -= 1/2 nu^2 / r_i; lw' = lw + ll, a
 *              non-finite lw' counts as -inf.  m = max lw', e_p = exp(lw'_p - m), eta = sum e_p;
 *              lw <- lw' - (m + ln eta), loglik += m + ln eta - 1/2 sum_present ln(2 pi r_i).  A step with no z present
 *              leaves lw untouched, bit for bit, and adds 0.  If no particle has a finite lw' the env's ok is 0,
 *              lw <- -ln P, every e_p counts as 1 and loglik is left alone.
 *   integer    wq_p = (uint32) rint(e_p 2^24): the heaviest particle has exactly 2^24.  Everything below uses wq in exact
 *   weights    64-bit integer arithmetic: S1 = sum wq, S2 = sum wq^2, ess = (double)S1 (double)S1 / (double)S2; the step
 *              resamples iff (double)S1 (double)S1 < (ess_frac P) (double)S2.
 *   estimate   (before resampling)  xhat = sum wq_p x_p / S1, var = sum wq_p (x_p - xhat)^2 / S1, particles of weight 0
 *              left out; best = the lowest index of the largest wq, status = that particle's.  The order of these
 *              sums is fixed (no atomics): the same inputs give the same bits on every call.
 *   resample   systematic: u = the top 16 bits of the step's resampling word, C_p the inclusive cumulative sum of wq;
 *              the ancestor of slot j is the smallest p with C_p (P << 16) > ((j << 16) + u) S1 (both sides < 2^61).
 *              Particle j takes its ancestor's state and status, lw <- -ln P.  Without a resample the ancestors are the
 *              identity.
 * Outputs, each may be NULL; var, ess, P and loglik in out_dtype (CS_JAC_F64, or CS_JAC_F32: the float64 values rounded):
 *   io->x_dev [K,N,12] float64 xhat     io->status_dev [K,N]        var_dev [K,N,12]         ess_dev [K,N]
 *   resampled_dev [K,N] uint8           best_dev [K,N] int32        P_dev [N,12,12] the weighted covariance after step
 *   loglik_dev [N]                      ok_dev [N] uint8            K, before its resampling (symmetric; diagonal = var)
 *   part_out_dev [N,P,12], pstatus_out_dev [N,P], lw_out_dev [N,P]: the state after step K, post-resample
 * and the tapes:
 *   part_tape_dev [K,N,P,12] the prior particles after the noise    pstatus_tape_dev [K,N,P] their statuses
 *   lw_tape_dev [K,N,P] normalised, before resampling               wq_tape_dev [K,N,P] uint32
 *   anc_tape_dev [K,N,P] int32
 * Refused (CS_ERR_ARG) under action_arith = CS_ARITH_F32.  Asynchronous on `stream`; pio->struct_size must be
 * sizeof(cs_rollout_pf_io) (else CS_ERR_ABI, checked first); both blocks are checked before the context.  r_dev must be
 * finite and > 0 (the caller's to guarantee; gym_copter_amd checks it).  Every array is aligned to its element size. */
#define CS_PF_MIN_PARTICLES 64
#define CS_PF_MAX_PARTICLES 1024
typedef struct cs_rollout_pf_io {
  uint32_t struct_size;            /* sizeof(cs_rollout_pf_io) */
  uint32_t out_dtype;              /* CS_JAC_F64 / CS_JAC_F32: var_dev, ess_dev, P_dev, loglik_dev */
  int32_t num_meas;                /* M, 1 .. CS_EKF_MAX_MEAS */
  int32_t num_particles;           /* P, a power of two in CS_PF_MIN_PARTICLES .. CS_PF_MAX_PARTICLES */
  uint32_t nonce;                  /* the second counter word of every draw */
  uint32_t first_step;             /* >= 1: the global index of the call's first step */
  double ess_frac;                 /* in [0, 1]: resample when ess < ess_frac P */
  const double* H_dev;             /* [M,12], required */
  const double* r_dev;             /* [M], required */
  const double* Lq_dev;            /* [12,12] lower triangular, required */
  const double* z_dev;             /* [K,N,M], required */
  const double* L0_dev;            /* [N,12,12] lower triangular, or NULL (Gaussian start) */
  const double* part_in_dev;       /* [N,P,12] (carried start) */
  const uint8_t* pstatus_in_dev;   /* [N,P] */
  const double* lw_in_dev;         /* [N,P] */
  void* var_dev;                   /* [K,N,12] */
  void* ess_dev;                   /* [K,N] */
  uint8_t* resampled_dev;          /* [K,N] */
  int32_t* best_dev;               /* [K,N] */
  void* P_dev;                     /* [N,12,12] */
  void* loglik_dev;                /* [N] */
  uint8_t* ok_dev;                 /* [N] */
  double* part_out_dev;            /* [N,P,12] */
  uint8_t* pstatus_out_dev;        /* [N,P] */
  double* lw_out_dev;              /* [N,P] */
  double* part_tape_dev;           /* [K,N,P,12] */
  uint8_t* pstatus_tape_dev;       /* [K,N,P] */
  double* lw_tape_dev;             /* [K,N,P] */
  uint32_t* wq_tape_dev;           /* [K,N,P] */
  int32_t* anc_tape_dev;           /* [K,N,P] */
} cs_rollout_pf_io;
int cs_rollout_pf(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_pf_io* pio, void* stream);

/* Output-feedback (LQG) rollouts on the device: cs_rollout_feedback_states' affine law evaluated
 * at the estimate of cs_rollout_ekf's filter, which predicts with the very action the law just chose -- truth, sensor,
 * filter and controller of K steps per env in one call.  Upstream lines composed: those of cs_rollout_states
 * (envs/task.py:77-137 step, dynamics/__init__.py:114-197 setMotors) for the truth and those of cs_rollout_ekf
 * (copterstep_jacobian.hip's: setMotors, the state derivative, step) for the filter.
 *
 * Per env, for step k = 1..K, in float64 without contraction, in this order:
 *   law      a_k = fl32( abar_k + sum_{j=0..11} K_k[c][j] (xhat_{k-1}[j] - xbar_{k-1}[j]) ) per motor c: from (double) abar,
 *            for j ascending one subtraction, one multiply and one add, never fused; one rounding to float32.  This is
 *            cs_rollout_feedback_states' arithmetic without alpha d, at the filter's posterior mean instead of the true
 *            state.  xhat_0 = xhat0_dev, the caller's starting estimate (step 1 has a deviation term); xbar_dev row k-1
 *            is the reference point BEFORE step k; abar = io->actions_dev.  a_k is stored unclipped to actions_out_dev
 *            (the step clips).
 *   truth    one step of cs_rollout_states under a_k from io's start point -- the stored env or io's explicit start with
 *            its pending force, a pending NEXT_STEP reset, prev_shaping, the step counter, the storage rounding of the
 *            mode; no env state is written.  Its tapes go to io's x_dev, reward_dev, terminated_dev, truncated_dev and
 *            status_dev (each may be NULL), bit-identical to cs_rollout_states fed actions_out_dev.
 *   measure  z_k[i] = sum_j H[i][j] x_k[j] + e_k[i], x_k the row written to x_dev; j ascending, the first product starts
 *            the sum, one multiply and one add per term, then one add of e.  e_dev is the caller's noise tape, already
 *            scaled by sqrt(r); a NaN entry means "no measurement" and yields a NaN z.  z is stored to z_dev (or NULL).
 *   filter   cs_rollout_ekf's predict under a_k (the same float32 value; the mean without storage rounding, P- = A P A^T
 *            + Q), then its M sequential scalar updates on z_k.  xhat_dev, fstatus_dev (the filter's own status; it may
 *            differ from the truth's), x_pred_dev, P_dev, P_tape_dev, var_dev, nis_dev, loglik_dev, branch_dev and ok_dev
 *            are cs_rollout_ekf's x, status, ... outputs, defined and rounded (out_dtype) as there; each may be NULL.
 * The truth has no process noise (its disturbance is the env's own perturbation force) and e is not drawn on the device.
 * Refused (CS_ERR_ARG) under action_arith = CS_ARITH_F32; io's cotangent and gradient pointers must be NULL.
 * Asynchronous on `stream`; lio->struct_size must be sizeof(cs_rollout_lqg_io) (else CS_ERR_ABI); both blocks are checked
 * before the context, with cs_rollout_ekf's alignment rules. */
typedef struct cs_rollout_lqg_io {
  uint32_t struct_size;        /* sizeof(cs_rollout_lqg_io) */
  uint32_t out_dtype;          /* CS_JAC_F64 / CS_JAC_F32: P_dev, P_tape_dev, var_dev, nis_dev, loglik_dev */
  int32_t num_meas;            /* M, 1 .. CS_EKF_MAX_MEAS */
  uint32_t reserved_;          /* 0 */
  const double* K_dev;         /* [K,N,A,12] float64, required */
  const double* xbar_dev;      /* [K,N,12] float64, required: row k-1 is the reference before step k */
  const double* e_dev;         /* [K,N,M] float64, required: the measurement noise, NaN = no measurement */
  const double* H_dev;         /* [M,12], required */
  const double* r_dev;         /* [M], required */
  const double* Q_dev;         /* [12,12], required */
  const double* P0_dev;        /* [N,12,12], required */
  const double* xhat0_dev;     /* [12,N], required: the starting estimate */
  const uint8_t* status0_dev;  /* [N], required: its flight status */
  float* actions_out_dev;      /* [K,N,A] float32, required */
  double* z_dev;               /* [K,N,M] */
  double* xhat_dev;            /* [K,N,12] */
  double* x_pred_dev;          /* [K,N,12] */
  void* P_dev;                 /* [N,12,12] */
  void* P_tape_dev;            /* [K,N,12,12] */
  void* var_dev;               /* [K,N,12] */
  void* nis_dev;               /* [K,N] */
  void* loglik_dev;            /* [N] */
  uint8_t* fstatus_dev;        /* [K,N] */
  uint8_t* branch_dev;         /* [K,N] */
  uint8_t* ok_dev;             /* [N] */
} cs_rollout_lqg_io;
int cs_rollout_lqg(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_lqg_io* lio, void* stream);

/* An unscented Kalman filter over the env step, on the device: K predict / update steps per env
 * in one call, between cs_rollout_ekf (one Jacobian at the mean's own branch) and cs_rollout_pf (64 to 1 024 sampled
 * particles): 2 * 12 + 1 = 25 deterministic sigma points per env, each through the step's own physics, no Jacobian.
 * The filter's state -- the mean xhat [12], the covariance P [12,12] and the flight status of the mean -- is the
 * CALLER's: no env state is read except the context's constants and vehicle table, and none is written.  The measurement
 * model, the process noise, io's fields and the update are cs_rollout_ekf's.  Upstream lines: those of cs_rollout_states,
 * per point.
 *
 * From io: as cs_rollout_ekf (num_steps, actions_dev, start_x_dev = xhat_0, start_status_dev; x_dev and status_dev
 * receive the filtered means and the status of the mean; everything else NULL).
 * From uio: num_meas, H_dev, r_dev, Q_dev, P0_dev, z_dev as cs_rollout_ekf's (P0 must be positive definite and Q should
 * be: the covariance is factored at every step), and the points' spread and weights
 *   gamma  finite, > 0     wm0, wc0, wi  finite (else CS_ERR_ARG)
 * For the scaled transform of (alpha, beta, kappa): lambda = alpha^2 (12 + kappa) - 12, gamma = sqrt(12 + lambda),
 * wm0 = lambda / (12 + lambda), wc0 = wm0 + 1 - alpha^2 + beta, wi = 1 / (2 (12 + lambda)); the call knows nothing of
 * them.  The prior's covariance below is the weighted covariance about the weighted mean when wm0 + 24 wi = 1, which
 * the scaled transform guarantees.
 * Per step k = 1..K and env, in float64 without contraction (the arithmetic of gym_copter_amd/csrc/ukf_points.h, which
 * tests/ukf_ref.py restates):
 *   landed    if the status of the mean is LANDED no points are made: x- = xhat, P- = P + Q with one add per entry.
 *   factor    else P = L L^T, L = U^T of cs_rollout_rts' Cholesky factorisation (column by column, the reciprocal root
 *             of a pivot kept; L[j][j] = 1 / that).  A pivot that is <= 0 or not finite clears the env's ok; the
 *             arithmetic is carried through and every output is written regardless.
 *   points    point 0 = xhat, point 1+j = xhat + gamma L[:,j], point 13+j = xhat - gamma L[:,j], j = 0 .. 11 (entries
 *             above the column's diagonal are xhat's own).
 *   propagate each point through the physics of step k under actions[k-1] from (the point, the status of the mean), as
 *             cs_rollout_ekf's mean goes: no storage rounding, no pending perturbation, a status variable of its own.
 *             In float64 storage a propagated point is cs_rollout_states' row from that explicit start bit for bit.  The
 *             filter's status after the step is point 0's.
 *   moments   with y_i the propagated points, sy = y_1 + .. + y_24 and S = sum_{i=1..24} (y_i - y_0)(y_i - y_0)^T summed
 *             in that order from zero:  x- = wm0 y_0 + wi sy;  m = x- - y_0;
 *             P- = (wi S - (2 - (wc0 + 24 wi)) m m^T) + Q, the upper triangle, Q last with one add per entry.
 *   update    cs_rollout_ekf's, with its nis, loglik and ok.
 * Outputs, each may be NULL; x_pred, P, P_tape, var, nis, loglik and ok as cs_rollout_ekf's (out_dtype likewise), and
 *   spread_dev       [K,N] uint8        how many of the 25 points ended the step with another status than point 0's
 *                                       (0 on a LANDED step)
 *   points_dev       [K,N,25,12] float64  the points before the physics      (for tests and diagnosis; on a LANDED
 *   points_pred_dev  [K,N,25,12] float64  ... and after it                    step all 25 rows hold xhat and the
 *   point_status_dev [K,N,25] uint8       their statuses after it             statuses are LANDED)
 * Refused (CS_ERR_ARG) under action_arith = CS_ARITH_F32.  Asynchronous on `stream`; uio->struct_size must be
 * sizeof(cs_rollout_ukf_io) (else CS_ERR_ABI); both blocks are checked before the context, with cs_rollout_ekf's
 * alignment rules. */
typedef struct cs_rollout_ukf_io {
  uint32_t struct_size;        /* sizeof(cs_rollout_ukf_io) */
  uint32_t out_dtype;          /* CS_JAC_F64 / CS_JAC_F32: P_dev, P_tape_dev, var_dev, nis_dev, loglik_dev */
  int32_t num_meas;            /* M, 1 .. CS_EKF_MAX_MEAS */
  uint32_t reserved_;          /* 0 */
  double gamma;                /* the points' spread, finite and > 0 */
  double wm0;                  /* the centre point's weight in the mean, finite */
  double wc0;                  /* the centre point's weight in the covariance, finite */
  double wi;                   /* every other point's weight, finite */
  const double* H_dev;         /* [M,12], required */
  const double* r_dev;         /* [M], required */
  const double* Q_dev;         /* [12,12], required */
  const double* P0_dev;        /* [N,12,12], required, positive definite */
  const double* z_dev;         /* [K,N,M], required */
  double* x_pred_dev;          /* [K,N,12] */
  void* P_dev;                 /* [N,12,12] */
  void* P_tape_dev;            /* [K,N,12,12] */
  void* var_dev;               /* [K,N,12] */
  void* nis_dev;               /* [K,N] */
  void* loglik_dev;            /* [N] */
  uint8_t* spread_dev;         /* [K,N] */
  uint8_t* ok_dev;             /* [N] */
  double* points_dev;          /* [K,N,25,12] */
  double* points_pred_dev;     /* [K,N,25,12] */
  uint8_t* point_status_dev;   /* [K,N,25] */
} cs_rollout_ukf_io;
int cs_rollout_ukf(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_ukf_io* uio, void* stream);

/* An unscented Rauch-Tung-Striebel fixed-interval smoother over the tapes of cs_rollout_ukf, on the device (DESIGN.md
 * section 25): what cs_rollout_rts is to cs_rollout_ekf.  The estimate of every step given the measurements of all K
 * steps, and that of the starting point, in one call of K backward steps per env.  Each backward step makes the filter's
 * 25 sigma points of that step again from the filter's own tapes and takes the cross-covariance of the points before and
 * after the physics in place of cs_rollout_rts' W = A P_f: no Jacobian, and a belief that straddles a touchdown, a crash
 * or the motor clip is smoothed over every branch its points land on.  No env state is read except the context's
 * constants and vehicle table, and none is written.
 *
 * Row k = 0 .. K-1 of a tape is the state after step k+1; "row -1" is the filter's starting point (x0, P0, status0).
 *
 * From io: as cs_rollout_rts (num_steps = K, actions_dev, start_x_dev = x0 and start_status_dev = status0, both required;
 * x_dev [K,N,12] or NULL receives the smoothed means; every other pointer NULL).
 * From sio, the inputs (float64): x_f_dev, x_pred_dev, status_f_dev, P_f_dev (the filter's x_dev, x_pred_dev, status_dev
 * and, with CS_JAC_F64, P_tape_dev), Q_dev, P0_dev, end_x_dev and end_P_dev as cs_rollout_rts'; gamma, wm0, wc0 and wi
 * as cs_rollout_ukf's -- they must be the filter's (gamma finite and > 0, the weights finite, else CS_ERR_ARG); and
 *   workspace_dev  [ceil(N / 64), CS_URTS_WORKSPACE_ROWS, 64] float64, required: scratch of the call, one column of
 *                  CS_URTS_WORKSPACE_ROWS values per env (and per padding lane of the last 64).  Its contents before the
 *                  call are ignored and after it are unspecified; it overlaps nothing else the call is given.
 * The smoothed row K-1 is given: the filter's own row K-1, or (end_x, the upper triangle of end_P, mirrored); it is
 * written out as it is.  Then for j = K-2 down to -1 and every env, in float64 without contraction:
 *   points    if status_f[j] is LANDED the filter made no points: W = P_f[j] and P- = P_f[j] + Q, one add per entry.
 *             Else step j+2 of cs_rollout_ukf is repeated: P_f[j] = L L^T, the 25 points in the filter's order, each
 *             through the physics under actions[j+1] from (the point, status_f[j]), their moments in the filter's order:
 *             P- is the filter's own prior of that step, bit for bit.  With dY[:, c] = y(1 + c) - y(13 + c), c = 0 .. 11,
 *             W = (wi gamma) dY L^T, each entry summed over L's columns in order (gym_copter_amd/csrc/urts_cross.h): the
 *             transpose of the cross-covariance sum_i wc_i (chi_i - x_f[j]) (y_i - x-)^T.  A pivot of this
 *             factorisation that is <= 0 or not finite clears the env's ok; the arithmetic is carried through.
 *   solve, smooth   cs_rollout_rts', with this W and x_pred[j+1] read from the filter's tape.
 * Outputs, each may be NULL: cs_rollout_rts' (io->x_dev, P_tape_dev, var_dev, x0_dev, P0_s_dev, ok_dev; P_tape, var and
 * P0_s in out_dtype).  No output may overlap an input.  Refused (CS_ERR_ARG) under action_arith = CS_ARITH_F32.
 * Asynchronous on `stream`; sio->struct_size must be sizeof(cs_urts_io) (else CS_ERR_ABI); both blocks are checked
 * before the context, with cs_rollout_rts' alignment rules. */
#define CS_URTS_WORKSPACE_ROWS 102 /* P_s [78] and x_s [12] of the row above, the filter's mean of this row [12] */
typedef struct cs_urts_io {
  uint32_t struct_size;        /* sizeof(cs_urts_io) */
  uint32_t out_dtype;          /* CS_JAC_F64 / CS_JAC_F32: P_tape_dev, var_dev, P0_s_dev */
  double gamma;                /* the filter's: the points' spread, finite and > 0 */
  double wm0;                  /* the filter's: the centre point's weight in the mean, finite */
  double wc0;                  /* the filter's: the centre point's weight in the covariance, finite */
  double wi;                   /* the filter's: every other point's weight, finite */
  const double* x_f_dev;       /* [K,N,12], required */
  const double* x_pred_dev;    /* [K,N,12], required */
  const uint8_t* status_f_dev; /* [K,N], required */
  const double* P_f_dev;       /* [K,N,12,12], required */
  const double* Q_dev;         /* [12,12], required */
  const double* P0_dev;        /* [N,12,12], required */
  const double* end_x_dev;     /* [12,N] or NULL */
  const double* end_P_dev;     /* [N,12,12] or NULL (with end_x_dev: both or neither) */
  double* workspace_dev;       /* [ceil(N / 64), CS_URTS_WORKSPACE_ROWS, 64], required */
  void* P_tape_dev;            /* [K,N,12,12] */
  void* var_dev;               /* [K,N,12] */
  double* x0_dev;              /* [12,N] */
  void* P0_s_dev;              /* [N,12,12] */
  uint8_t* ok_dev;             /* [N] */
} cs_urts_io;
int cs_urts_smooth(cs_ctx* ctx, const cs_rollout_io* io, const cs_urts_io* sio, void* stream);

/* A backward-simulation particle smoother over the tapes of cs_rollout_pf, on the device: forward
 * filtering, backward simulation.  S trajectories ("paths") per env are drawn backwards through the filter's taped
 * particle sets; every earlier particle is reweighted by its filter weight times the transition density to the path's
 * next point.  What cs_rollout_rts is to cs_rollout_ekf, for the filter that keeps a belief on both sides of a branch
 * of the step.  No env state is read except the context's constants and vehicle table, and none is written.  Everything
 * is float64 without contraction unless stated.
 *
 * From io: num_steps = K, actions_dev [K,N,A] (the filter's), x_dev [K,N,12] or NULL (the smoothed means); every other
 * pointer of io must be NULL.  From sio, per env and row k = 0 .. K-1 (row k is the filter's step first_step + k):
 *   X_k[i] = part_tape_dev[k,env,i] (the prior particles), s_k[i] = pstatus_tape_dev[k,env,i], lw_k[i] =
 *   lw_tape_dev[k,env,i], wq_tape_dev (read at row K-1 only, and only without end_idx_dev): the filter's tapes;
 *   Linv_dev [12,12]: the inverse of the filter's Lq, lower triangular (the upper triangle is not read);
 *   P = num_particles (the filter's), S = num_paths in 1 .. CS_PFS_MAX_PATHS, nonce, first_step (the filter's).
 *
 * Row K-1.  b[K-1,m] = end_idx_dev[env,m] mod P when end_idx_dev is given, else drawn (below) from the integer weights
 *   wq_tape[K-1].
 * For k = K-2 down to 0:
 *   (mu_i, sigma_i) is the physics of step k+1 from (X_k[i], s_k[i]) under actions[k+1], without noise: the code
 *   cs_rollout_pf propagates with (clip, motor law, the env's vehicle, `substeps` calls, the status machine, skipped for
 *   a LANDED particle) -- mu_i is cs_rollout_states' row from that point, bit for bit in float64 storage.
 *   y_i = Linv mu_i: row r is sum_{j <= r} Linv[r][j] mu_i[j], j ascending, the first term starting the sum, one multiply
 *   and one add per term (gym_copter_amd/csrc/pfs_draw.h).
 *   For path m: xt = X_{k+1}[b[k+1,m]], st = s_{k+1}[b[k+1,m]], yt = Linv xt;
 *     d2 = sum_j (yt_j - y_i,j)^2, j ascending, the first term starting the sum;
 *     logb_i = lw_k[i] + (-0.5 d2) if sigma_i == st, else -inf: the flight status is a deterministic part of the
 *     transition.  A non-finite value counts as -inf.
 *     mx = max_i logb_i.  If mx is -inf the env's ok is 0 and e_i = 1 for every i (as the filter's dead step); else
 *     e_i = exp(logb_i - mx).  bwq_i = (uint32) rint(e_i 2^24), and b[k,m] is drawn from bwq.
 * Row -1 (optional).  With a start set part_in_dev [N,P,12], pstatus_in_dev [N,P], lw_in_dev [N,P] (all three or none:
 *   the prior particles of the step before this call's first, rows of the filter's tapes) one more backward step is made
 *   from it under actions[0]; its indices go to idx0_dev [N,S].  A tape is smoothed in chunks, last chunk first, by
 *   passing a later chunk's idx0 as the earlier chunk's end_idx.
 * Draw.  With C the inclusive cumulative sum of the integer weights, S1 = C[P-1] and u = the top 24 bits of the first
 *   Philox word of (g, nonce, kg, m, slot 13) of cs_rollout_pf's noise -- kg = first_step + k is the global index of the
 *   row being drawn (first_step - 1 for row -1), the path m stands in the key's particle field -- the index is the
 *   smallest p with (C[p] << 24) > u S1 (both sides < 2^58); P - 1 if every weight is 0.  A pure function of the seed,
 *   the global env id, the nonce, the global row and the path: it does not depend on S, P, the batch, the sharding or
 *   the chunking.
 * Estimates per row, equal weights over the S paths: the mean of X_k[b[k,m]] and the variance about that mean (summed
 *   and divided by S).  The order of the sums is fixed (no atomics): the same inputs give the same bits on every call.
 * Outputs, each may be NULL; var in out_dtype (CS_JAC_F64, or CS_JAC_F32: the float64 values rounded):
 *   idx_dev [K,N,S] int32 = b          io->x_dev [K,N,12] float64      var_dev [K,N,12]
 *   idx0_dev [N,S] int32 (needs the start set, else CS_ERR_ARG)        ok_dev [N] uint8
 * and two diagnostic tapes:
 *   logb_tape_dev [K,N,S,P] float64: logb of rows 0 .. K-2; row K-1 holds lw_tape[K-1] (for every path) when it is
 *                 drawn, and is NOT written when end_idx_dev is given
 *   bwq_tape_dev [K,N,S,P] int32: bwq of rows 0 .. K-2; row K-1 holds wq_tape[K-1] when it is drawn, and is NOT written
 *                 when end_idx_dev is given
 * No output may overlap an input.  Refused (CS_ERR_ARG) under action_arith = CS_ARITH_F32.  Asynchronous on `stream`;
 * sio->struct_size must be sizeof(cs_pf_smooth_io) (else CS_ERR_ABI, checked first); both blocks are checked before the
 * context.  Every array is aligned to its element size. */
#define CS_PFS_MAX_PATHS 1024
typedef struct cs_pf_smooth_io {
  uint32_t struct_size;            /* sizeof(cs_pf_smooth_io) */
  uint32_t out_dtype;              /* CS_JAC_F64 / CS_JAC_F32: var_dev */
  int32_t num_particles;           /* P, the filter's: a power of two in CS_PF_MIN_PARTICLES .. CS_PF_MAX_PARTICLES */
  int32_t num_paths;               /* S, 1 .. CS_PFS_MAX_PATHS */
  uint32_t nonce;                  /* the second counter word of every draw */
  uint32_t first_step;             /* >= 1: the global index of row 0's step (the filter's first_step) */
  const double* part_tape_dev;     /* [K,N,P,12], required */
  const uint8_t* pstatus_tape_dev; /* [K,N,P], required */
  const double* lw_tape_dev;       /* [K,N,P], required */
  const uint32_t* wq_tape_dev;     /* [K,N,P], required without end_idx_dev */
  const double* Linv_dev;          /* [12,12] lower triangular, required */
  const int32_t* end_idx_dev;      /* [N,S] or NULL */
  const double* part_in_dev;       /* [N,P,12] (the start set: all three or none) */
  const uint8_t* pstatus_in_dev;   /* [N,P] */
  const double* lw_in_dev;         /* [N,P] */
  int32_t* idx_dev;                /* [K,N,S] */
  void* var_dev;                   /* [K,N,12] */
  int32_t* idx0_dev;               /* [N,S] */
  uint8_t* ok_dev;                 /* [N] */
  double* logb_tape_dev;           /* [K,N,S,P] */
  int32_t* bwq_tape_dev;           /* [K,N,S,P] */
} cs_pf_smooth_io;
int cs_pf_smooth(cs_ctx* ctx, const cs_rollout_io* io, const cs_pf_smooth_io* sio, void* stream);

/* MPPI (model-predictive path integral control) on the device: zeroth-order, sampling-based
 * trajectory optimisation, which sees across the branches of the step that have no useful derivative (touchdown, crash,
 * tilt, the motor clip).  For every env, P perturbed copies of the nominal action tape abar = io->actions_dev [K,N,A] are
 * rolled out for K steps and scored (cs_rollout_mppi_costs); the cost-weighted average of the perturbations then replaces
 * the nominal (cs_rollout_mppi_update).  Neither the states nor the noise touch memory: the cost accumulates in registers,
 * and the noise is a counter-based draw that the update makes again.
 *
 * Noise.  Sample p in [0, P), step k in [1, K], action component j in [0, A), the env with global id g (cs_config.
 * env_id_base + local index), the caller's nonce mio->noise_stream (for example the MPC iteration): ONE Philox2x32-10
 * call with counter = (g, noise_stream) and key = key_noise + (((k - 1) << 16) + p) * 4 + j (mod 2^32) gives 64 bits;
 * key_noise = lo32(splitmix64(splitmix64(seed))), a third mix of the seed beside the two keys of cs_seed.  Its four
 * 16-bit halves u0..u3 give the exact integer T = u0 + u1 + u2 + u3 - 131070 and
 *     eps = (float)T * CS_MPPI_NOISE_SCALE          (one float32 multiply; CS_MPPI_NOISE_SCALE = fl32(sqrt(3) 2^-16))
 * -- Irwin-Hall of order 4: mean 0, variance 1 - 2^-32, support +-3.46.  It is a pure function of (seed, g, noise_stream,
 * k, p, j): independent of the batch size, the sharding, P and the launch history (keys are distinct for k <= 16 384).
 * Sample actions.  a(p)[k][j] = abar[k][j] + sigma[j] * eps(p, k, j) in float32, one multiply and one add, not fused;
 * sample 0 is the nominal itself, a(0) = abar bit for bit, so costs[0] is the cost of the unperturbed plan.  sigma_dev [A]
 * float32, each >= 0 (the caller's to guarantee), shared by all envs.  The step clips motors to [0, 1] itself, as always.
 * Cost.  With x_k, reward_k what cs_rollout_states returns for that action tape from the same start, in float64 without
 * contraction,
 *     S = sum_{k=1..K} [ 1/2 (x_k - xref_k)^T Q_k (x_k - xref_k) + 1/2 (a_k - aref)^T R (a_k - aref) - w_r reward_k ]
 * Q_k = Q_dev [12,12], Q_final_dev at k = K when given; R_dev [A,A]; both symmetric (their upper triangles are read),
 * shared; a_k is the sample's float32 action before the clip; aref = a_ref_dev [A] float64 or NULL = 0; xref = x_ref_dev,
 * [N,12] (x_ref_steps = 0) or [K,N,12] (x_ref_steps = 1); w_r = reward_weight >= 0 brings in the task's own reward.
 *
 * cs_rollout_mppi_costs writes costs_dev [P,N] float64 and, when best_dev != NULL, best_dev [N] int32: the arg-min over
 * the finite costs of the env, the lowest index on ties, -1 if none is finite.  The start point -- stored or explicit, the
 * pending perturbation, a pending NEXT_STEP reset, the step counter -- is cs_rollout_states'; io's outputs, cotangents and
 * gradients are not used.  No env state is written.
 * cs_rollout_mppi_update reads costs_dev [P,N] and, per env: beta = the minimum finite cost; w_p = exp(-(S_p - beta) /
 * lambda) for a finite S_p, else 0; eta = sum_p w_p;
 *     actions_out[k][j] = clip01( fl32( (double)abar[k][j] + (1 / eta) sum_p w_p (double)(sigma[j] * eps(p, k, j)) ) )
 * with float64 sums over p ascending (sigma[j] * eps is the float32 product of the sample actions; the p = 0 term is 0)
 * and eps drawn again from the counter.  It writes actions_out_dev [K,N,A] float32 (must not alias io->actions_dev),
 * ess_dev [N] float64 = eta^2 / sum_p w_p^2 and cost_min_dev [N] = beta (each of the two may be NULL).  An env without a
 * finite cost keeps its abar (the same bits) and reports ess = 0, cost_min = +inf.  lambda > 0, finite.  The call reads
 * io->actions_dev and io->num_steps only (the start point plays no part); P, sigma and noise_stream must be those of the
 * cs_rollout_mppi_costs call that made costs_dev.
 * Every reduction runs inside one lane in a fixed order (no atomics, no cross-lane sums): two calls give the same bits.
 * P <= CS_MPPI_MAX_SAMPLES and (update) K <= CS_MPPI_MAX_SAMPLES: the sample and step indices are the launch grid's y.
 * Asynchronous on `stream`; mio->struct_size must be sizeof(cs_rollout_mppi_io) (else CS_ERR_ABI); both blocks are
 * checked before the context.  The shared matrices are read by the scalar unit: 8-B aligned (sigma_dev 4-B), never
 * written while a call runs; x_ref_dev is 16-B aligned. */
#define CS_MPPI_MAX_SAMPLES 65535
#define CS_MPPI_NOISE_SCALE 0x1.bb67aep-16f
typedef struct cs_rollout_mppi_io {
  uint32_t struct_size;        /* sizeof(cs_rollout_mppi_io) */
  int32_t num_samples;         /* P in [1, CS_MPPI_MAX_SAMPLES] */
  uint32_t noise_stream;       /* the nonce of the noise */
  uint32_t x_ref_steps;        /* 0: x_ref_dev is [N,12]; 1: [K,N,12] */
  double lam;                  /* update: lambda, the temperature, > 0 and finite */
  double reward_weight;        /* costs: w_r >= 0, finite */
  const float* sigma_dev;      /* [A] float32, required */
  const double* x_ref_dev;     /* costs: required */
  const double* a_ref_dev;     /* costs: [A] float64 or NULL = zero */
  const double* Q_dev;         /* costs: [12,12], required */
  const double* Q_final_dev;   /* costs: [12,12] or NULL */
  const double* R_dev;         /* costs: [A,A], required */
  double* costs_dev;           /* [P,N]: written by _costs, read by _update (required) */
  int32_t* best_dev;           /* costs: [N] or NULL */
  float* actions_out_dev;      /* update: [K,N,A], required */
  double* ess_dev;             /* update: [N] or NULL */
  double* cost_min_dev;        /* update: [N] or NULL */
} cs_rollout_mppi_io;
int cs_rollout_mppi_costs(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_mppi_io* mio, void* stream);
int cs_rollout_mppi_update(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_mppi_io* mio, void* stream);

/* MPPI with smooth knot noise and a per-env temperature.  cs_rollout_mppi_costs_ex and
 * cs_rollout_mppi_update_ex are cs_rollout_mppi_costs and cs_rollout_mppi_update -- the same io and mio, the same
 * outputs, the same rules -- with the noise law and the temperature taken from a second block, cs_rollout_mppi_ext.
 *
 * Noise.  Per step k = 1..K the caller gives a knot number knot_dev[k-1] >= 1 and two float32 weights
 * knot_weights_dev[k-1][0..1].  With eps(p, m, j) the draw above made with the knot number m in its step slot,
 *     eps~(p, k, j) = fl32( fl32(w[k][0] * eps(p, knot[k], j)) + fl32(w[k][1] * eps(p, knot[k] + 1, j)) )
 * two float32 multiplies and one add, none fused; the second term is left out altogether when w[k][1] == 0.  The sample
 * action and the update's perturbation use fl32(sigma[j] * eps~) exactly where they use fl32(sigma[j] * eps) above;
 * sample 0 stays the nominal bit for bit.  knot[k] = k with w = (1, 0) is the white noise above, and both calls then
 * give the bits of cs_rollout_mppi_costs / cs_rollout_mppi_update; so they do with knot_dev and knot_weights_dev both
 * NULL (one without the other is CS_ERR_ARG).  The caller guarantees knot[k] + 1 <= 16 384 (the keys stay distinct), as
 * it guarantees sigma >= 0.  Neighbouring steps that share a knot pair are correlated: w = (1 - t, t) / |(1 - t, t)| over
 * a hold of h steps, t = ((k - 1) mod h) / h, is a piecewise-linear tape of unit variance at every step.
 * Temperature.  cs_rollout_mppi_update_ex reads lam_dev [N] float64 when it is not NULL: env i weighs its samples with
 * lambda = lam_dev[i] in place of mio->lam (which is then not looked at).  An entry that is not finite and > 0 leaves
 * that env's plan unchanged (the same bits) and reports ess = 0; cost_min is beta as ever.
 * cs_rollout_mppi_temperature solves that lambda per env, on the device, for a target effective sample size.  It
 * reads mio->num_samples and mio->costs_dev [P,N] only (and checks mio as the other calls do, sigma_dev apart).  With
 * E(lambda) = (sum_p w_p)^2 / sum_p w_p^2 over the finite costs, the weights above, sums over p ascending in float64:
 * u_lo = ln lam_min, u_hi = ln lam_max; 48 times u = (u_lo + u_hi) / 2, and u_lo = u if E(exp u) < ess_target, else
 * u_hi = u; the result is lambda = exp(u_hi).  lambda = lam_max where E(lam_max) < ess_target; lambda = lam_min where
 * E(lam_min) >= ess_target; an env without a finite cost gets lambda = lam_max and E = 0.  It writes lam_out_dev [N]
 * (required) and, when not NULL, ess_out_dev [N] = E(lambda).  ess_target >= 1 and 0 < lam_min < lam_max, all finite.
 * Every sum runs inside one lane in a fixed order: two calls give the same bits.
 * ext->struct_size must be sizeof(cs_rollout_mppi_ext) (else CS_ERR_ABI) and ext->reserved_ 0; all three blocks are
 * checked before the context.  knot_dev and knot_weights_dev are 4-B aligned and never written while a call runs.
 * Asynchronous on `stream`; no env state is written. */
typedef struct cs_rollout_mppi_ext {
  uint32_t struct_size;            /* sizeof(cs_rollout_mppi_ext) */
  uint32_t reserved_;              /* 0 */
  const uint32_t* knot_dev;        /* costs_ex, update_ex: [K] or NULL (with knot_weights_dev) = white noise */
  const float* knot_weights_dev;   /* costs_ex, update_ex: [K,2] float32 or NULL */
  const double* lam_dev;           /* update_ex: [N] float64 or NULL = mio->lam */
  double ess_target;               /* temperature: >= 1, finite */
  double lam_min;                  /* temperature: 0 < lam_min < lam_max, finite */
  double lam_max;
  double* lam_out_dev;             /* temperature: [N], required */
  double* ess_out_dev;             /* temperature: [N] or NULL */
} cs_rollout_mppi_ext;
int cs_rollout_mppi_costs_ex(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_mppi_io* mio,
                             const cs_rollout_mppi_ext* ext, void* stream);
int cs_rollout_mppi_update_ex(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_mppi_io* mio,
                              const cs_rollout_mppi_ext* ext, void* stream);
int cs_rollout_mppi_temperature(cs_ctx* ctx, const cs_rollout_mppi_io* mio, const cs_rollout_mppi_ext* ext,
                                void* stream);

/* Population rollouts and evolution strategies for the MLP policy: M parameter vectors, each
 * rolled out closed-loop on its own E envs and scored by its episode return, without a tape; the mirrored population
 * around a centre, and the search gradient of its shaped fitness, on the device.
 *
 * cs_rollout_mlp_population.  N = members x envs_per_member (else CS_ERR_ARG), envs_per_member a multiple of 64; env i
 * belongs to member i / E and runs under theta = params_table_dev[i / E] ([M,P] float32, every row in
 * cs_rollout_mlp_io's layout for `hidden`).  io gives the start and K as it does for cs_rollout_mlp_states (stored or
 * explicit start, the pending perturbation, a pending NEXT_STEP reset, the step counter; io->actions_dev must be NULL,
 * its outputs, cotangents and gradients are not used).  With reward_k, terminated_k, truncated_k, status_k what
 * cs_rollout_mlp_states returns for that start with params_dev = the member's row and no offsets, and d = the first
 * step k in 1..K with terminated_k or truncated_k set, or K if there is none:
 *   returns_dev     [N] float64  sum_{k=1..d} disc_k reward_k: k ascending from 0.0, every product and every sum rounded
 *                                on its own (no contraction), disc_1 = 1, disc_{k+1} = fl64(disc_k x gamma)   (required)
 *   lengths_dev     [N] int32    d
 *   end_flags_dev   [N] uint8    bit 0: terminated_d, bit 1: truncated_d
 *   end_status_dev  [N] uint8    status_d (CS_STATUS_*)
 * each of the last three may be NULL.  A lane with a NEXT_STEP reset pending performs that reset in step 1 (reward 0,
 * no flag) and goes on with the new episode, as in cs_rollout_mlp_states.  The policy's float32 arithmetic is
 * cs_rollout_mlp_states' bit for bit, so all four outputs are exactly what the tapes give.  No env state and no tape is
 * written; a wavefront whose 64 envs are all past d leaves the step loop.
 *   member_returns_dev [M] float64 or NULL: the mean of returns over the member's E envs, by a second kernel: lane l of
 * the member's wavefront adds returns[m E + l + 64 t] for t = 0, 1, .. in that order from 0.0; then for off = 32, 16, 8,
 * 4, 2, 1 lane l adds the sum of lane l + off (lanes below off only: a binary tree); the result is lane 0's sum / E.
 * No atomics: the same inputs give the same bits on every call.
 * pio->struct_size must be sizeof(cs_rollout_population_io) (else CS_ERR_ABI); both blocks are checked before the
 * context, N = M E with it.  The table is read by the scalar unit: 4-B aligned, never written while a call runs.
 * gamma is finite.  Asynchronous on `stream`. */
typedef struct cs_rollout_population_io {
  uint32_t struct_size;           /* sizeof(cs_rollout_population_io) */
  int32_t hidden;                 /* 0 .. CS_MLP_MAX_HIDDEN */
  int32_t members;                /* M >= 1 */
  int32_t envs_per_member;        /* E: a positive multiple of 64 */
  double gamma;                   /* the discount, finite */
  const float* params_table_dev;  /* [M,P] float32, required */
  double* returns_dev;            /* [N], required */
  int32_t* lengths_dev;           /* [N] or NULL */
  uint8_t* end_flags_dev;         /* [N] or NULL */
  uint8_t* end_status_dev;        /* [N] or NULL */
  double* member_returns_dev;     /* [M] or NULL */
} cs_rollout_population_io;
int cs_rollout_mlp_population(cs_ctx* ctx, const cs_rollout_io* io, const cs_rollout_population_io* pio, void* stream);

/* The mirrored population of an evolution strategy and its search gradient.  Noise: pair i = 0 .. M/2 - 1 of a call has
 * the global pair index g = pair_base + i (mod 2^32); eps(g, p) for parameter p is ONE Philox2x32-10 call with counter =
 * (g, noise_stream) and key = key_es + p (mod 2^32), key_es = lo32(splitmix64(splitmix64(splitmix64(seed)))): a fourth
 * mix of the context's seed beside the two keys of cs_seed and the MPPI key.  The 64 bits give eps exactly as the MPPI
 * draw above: eps = (float)(u0 + u1 + u2 + u3 - 131070) * CS_MPPI_NOISE_SCALE, Irwin-Hall of order 4, mean 0, variance
 * 1 - 2^-32.  eps is a pure function of (seed, noise_stream, g, p): independent of M, P, of how a population is split
 * over calls (pair_base) and of the launch history; g and noise_stream are full 32-bit numbers, p < 2^32.
 *
 * cs_es_perturb writes table_dev [M,P] float32 from the centre params_dev [P]:
 *     table[2i][p] = fl32( theta[p] + fl32(sigma * eps(g, p)) ),  table[2i+1][p] = fl32( theta[p] - fl32(sigma * eps(g, p)) )
 * one float32 multiply and one add (subtract), not fused.  sigma >= 0 and finite; sigma = 0 gives M copies of theta.
 * cs_es_gradient writes grad_dev [P] float64 from the caller's weights_dev [M] float64 (the shaped fitness):
 *     g[p] = sum_{i} (w[2i] - w[2i+1]) * (double)eps(g_i, p)
 * with eps drawn again (neither the table nor theta is read), every difference, product and sum rounded on its own.  The
 * order is fixed: pairs in chunks of CS_ES_PAIR_CHUNK, i ascending from 0.0 inside a chunk, then the chunks' partial
 * sums added in chunk order from 0.0.  No floating-point atomics: the same inputs give the same bits on every call, and
 * grad_dev is WRITTEN, not accumulated.  The scale (1 / (M sigma) for the usual estimator) is the caller's.  The partial
 * sums live in a scratch of the context (8.9 MB, allocated by the first cs_es_gradient call on it: make that call outside
 * graph capture; released by cs_destroy): cs_es_gradient calls on one context must be ordered on one stream.
 * M is even, 2 <= M <= CS_ES_MAX_MEMBERS; 1 <= num_params <= CS_ES_MAX_PARAMS (the largest policy of cs_rollout_mlp_io).
 * eio->struct_size must be sizeof(cs_es_io) (else CS_ERR_ABI); the block is checked before the context.  Asynchronous on
 * `stream`; no env state is read or written. */
#define CS_ES_PAIR_CHUNK 32
#define CS_ES_MAX_MEMBERS 65536
#define CS_ES_MAX_PARAMS 1092
typedef struct cs_es_io {
  uint32_t struct_size;        /* sizeof(cs_es_io) */
  int32_t members;             /* M: even, in [2, CS_ES_MAX_MEMBERS] */
  int32_t num_params;          /* P in [1, CS_ES_MAX_PARAMS] */
  uint32_t noise_stream;       /* the nonce of the noise */
  uint32_t pair_base;          /* the global index of this call's pair 0 */
  float sigma;                 /* perturb: >= 0, finite */
  const float* params_dev;     /* perturb: [P] theta, required */
  float* table_dev;            /* perturb: [M,P], required */
  const double* weights_dev;   /* gradient: [M], required */
  double* grad_dev;            /* gradient: [P], required */
} cs_es_io;
int cs_es_perturb(cs_ctx* ctx, const cs_es_io* eio, void* stream);
int cs_es_gradient(cs_ctx* ctx, const cs_es_io* eio, void* stream);

/* On-policy actor-critic collection and generalised advantage estimation: what a PPO or A2C
 * learner needs of K closed-loop steps, in one launch, with the env in registers between the steps.
 *
 * cs_rollout_actor_critic runs K = num_steps steps under the env's own auto-reset mode and ADVANCES the stored state
 * exactly as cs_step_many would under the same actions (the step is the one cs_step runs).  With o_{k-1} the float32
 * observation the previous step returned (k = 1: that of the stored state), per step k = 1..K:
 *     mu  = pi_actor(o_{k-1})    cs_rollout_mlp_io's policy and float32 arithmetic (fmaf chains from the bias in index
 *                                order, the device library's tanhf, nothing contracted), hidden in 0 .. CS_MLP_MAX_HIDDEN
 *     V   = pi_critic(o_{k-1})   the same arithmetic with A = 1 and critic_hidden (critic_dev NULL: no values)
 *     a_c = fl32( mu_c + fl32(sigma_c * eps_c) ),  sigma_c = expf(log_std[c]) in float32: one multiply and one add, not
 *                                fused; with `deterministic` != 0, a = mu and no noise is drawn
 *     logp = -1/2 sum_c z_c^2 - sum_c log_std[c] - (A/2) ln(2 pi) in float64, c ascending, stored as float32, with
 *                                z_c = ((double)a_c - (double)mu_c) * exp(-(double)log_std[c]): computed from the
 *                                STORED action, so a learner that recomputes it from the tapes gets the ratio 1
 * then the step with that action.  Noise: eps of (g, nonce, k, c), g = the global env id the reset draw uses (sharding
 * cannot change a draw): ONE Philox2x32-10 call per pair of components with counter = (g, nonce) and key = key_pi + 2 k +
 * (c >> 1) (mod 2^32), key_pi = lo32(splitmix64^4(seed)): a fifth mix of the context's seed beside the two keys of cs_seed,
 * the MPPI key and the ES key.  With m1, m2 the top 24 bits of the two output words, in float32: u1 = (m1 + 0.5) 2^-24,
 * u2 = m2 2^-24, R = sqrtf(-2 logf(u1)), eps_even = R cosf(2 pi u2), eps_odd = R sinf(2 pi u2) -- Box-Muller: a true
 * Gaussian, a pure function of (seed, nonce, g, k, c), independent of N, K and the launch history.  u1 and u2 are
 * reproducible bit for bit, eps to the device library's logf / sinf / cosf accuracy.
 * Outputs, [K..] row blocks, every pointer 16-B aligned:
 *   obs_dev     [K+1,N,OBS] float32  row 0 = the stored state's observation, row k = what step k returned (required)
 *   actions_dev [K,N,A] float32      the action taken                                                      (required)
 *   means_dev   [K,N,A] float32      mu, or NULL
 *   logp_dev    [K,N] float32        as above                                                               (required)
 *   values_dev  [K+1,N] float32      row k = V(obs row k), k = 0..K; required with critic_dev, else must be NULL
 *   reward_dev  [K,N] float32        as cs_step_many                                                        (required)
 *   flags_dev   [K,N,2] uint8        terminated, truncated interleaved                                      (required)
 *   live_dev    [K,N] uint8          0 for a CS_AUTORESET_NEXT_STEP reset step (the env ignores its action, the reward is
 *                                    0), else 1: always 1 under SAME_STEP and with auto-reset disabled         (required)
 * aio->struct_size must be sizeof(cs_rollout_ac_io) (else CS_ERR_ABI); the block is checked before the context.  An
 * open served session is refused, and so are packed rows (reward_dev == obs_dev + OBS ...: cs_step_io).  The weights
 * are read by the scalar unit: 4-B aligned, never written while a call runs.  Asynchronous on `stream`. */
typedef struct cs_rollout_ac_io {
  uint32_t struct_size;        /* sizeof(cs_rollout_ac_io) */
  int32_t num_steps;           /* K >= 1 */
  int32_t hidden;              /* the actor's, 0 .. CS_MLP_MAX_HIDDEN */
  int32_t critic_hidden;       /* the critic's, 0 .. CS_MLP_MAX_HIDDEN */
  uint32_t nonce;              /* the nonce of the noise */
  uint32_t deterministic;      /* 0: sample, 1: a = mu */
  const float* actor_dev;      /* [P] float32, cs_rollout_mlp_io's layout, required */
  const float* critic_dev;     /* [Pv] float32, the same layout with A = 1, or NULL */
  const float* log_std_dev;    /* [A] float32, required */
  float* obs_dev;              /* [K+1,N,OBS] */
  float* actions_dev;          /* [K,N,A] */
  float* means_dev;            /* [K,N,A] or NULL */
  float* logp_dev;             /* [K,N] */
  float* values_dev;           /* [K+1,N], with critic_dev */
  float* reward_dev;           /* [K,N] */
  uint8_t* flags_dev;          /* [K,N,2] */
  uint8_t* live_dev;           /* [K,N] */
} cs_rollout_ac_io;
int cs_rollout_actor_critic(cs_ctx* ctx, const cs_rollout_ac_io* aio, void* stream);

/* Generalised advantage estimation over the tapes above, one kernel: lane = env, k descending, float32 in a fixed order
 * with every operation rounded on its own (no fma), so that NumPy float32 reproduces both outputs bit for bit:
 *     nd_k  = 1 - (terminated_k | truncated_k)
 *     delta = (r_k + (g * V_{k+1}) * nd_k) - V_k
 *     adv_k = delta + ((gl * nd_k) * adv_{k+1}),  adv_{K+1} = 0
 *     ret_k = adv_k + V_k
 * with g = fl32(gamma) and gl = fl32(fl32(gamma) * fl32(lam)), rounded once on the host.  A truncated step cuts the
 * bootstrap exactly as a terminated one does (the K-step forms return no final observation to bootstrap from).
 * N is the context's; terminated_dev / truncated_dev are [K,N] uint8 with `flag_stride` bytes between an env's and the
 * next env's flag: 1 = two plain arrays, 2 = the two columns of one interleaved [K,N,2] array.  gamma and lam are finite.
 * gio->struct_size must be sizeof(cs_gae_io) (else CS_ERR_ABI); the block is checked before the context.  No env state is
 * read or written; no atomics.  Asynchronous on `stream`. */
typedef struct cs_gae_io {
  uint32_t struct_size;          /* sizeof(cs_gae_io) */
  int32_t num_steps;             /* K >= 1 */
  uint32_t flag_stride;          /* 1 or 2 */
  uint32_t reserved_;            /* 0 */
  double gamma;
  double lam;
  const float* reward_dev;       /* [K,N], required */
  const float* values_dev;       /* [K+1,N], required */
  const uint8_t* terminated_dev; /* [K,N] (stride flag_stride), required */
  const uint8_t* truncated_dev;  /* [K,N] (stride flag_stride), required */
  float* advantages_dev;         /* [K,N], required */
  float* returns_dev;            /* [K,N], required */
} cs_gae_io;
int cs_gae(cs_ctx* ctx, const cs_gae_io* gio, void* stream);

/* The clipped-surrogate minibatch loss of PPO and its gradient over the tapes above: what
 * gym_copter_amd.ppo's minibatch step differentiates, evaluated in float64 from the float32 tapes and parameters.
 *
 * R = num_rows rows, row-major ([K,N] flattened, or any other row set): obs_dev [R,OBS], actions_dev [R,A], logp_dev [R],
 * advantages_dev [R], returns_dev [R] float32, live_dev [R] uint8 (NULL: every row live).  OBS and A are the context's
 * task's; the context supplies the shape, the device, the stream rules and the scratch, and no env state is read or
 * written.  The minibatch is B = num_samples samples: sample s is row index_dev[s] (int64, what a slice of
 * torch.randperm is), or row row_base + s with index_dev NULL.  A sample whose row is < 0 or >= R is skipped IN THE KERNEL
 * (weight 0, counted nowhere, nothing read); duplicates count as often as they occur.
 *
 * With i the row of sample s, w = (live[i] != 0) (any nonzero byte is live; a dead row, like a row the minibatch does not
 * name, is never read), W = max(sum w, 1), and, with `normalize`, m = sum w adv / W,
 * sd = sqrt(sum w (adv - m)^2 / W) (the centred form) and Ahat = (adv - m) / (sd + 1e-8), else Ahat = adv:
 *     mu = pi_actor(o_i), V = pi_critic(o_i)   cs_rollout_mlp_io's layout, the weights widened to double; the hidden
 *                                 units are fma chains from the bias in index order and the device library's double
 *                                 tanh, the outputs the bias plus a fixed pairwise tree over the hidden units
 *                                 (hidden = 0: an fma chain from the bias); nothing contracted
 *     z_c = (a_c - mu_c) exp(-ls_c),  logp = -1/2 sum_c z_c^2 - sum_c ls_c - (A/2) ln(2 pi), c ascending
 *     rho = exp(logp - logp_old); a sample is CLIPPED iff (Ahat > 0 and rho > 1 + clip) or (Ahat < 0 and rho < 1 - clip)
 *     L_pi = -(1/W) sum w Ahat (clipped ? clamp(rho, 1 - clip, 1 + clip) : rho)
 *     L_V  = (1/2W) sum w (V - ret)^2,   H = sum_c ls_c + A (1 + ln(2 pi)) / 2,   L = L_pi + vf_coef L_V - ent_coef H
 * grad_dev [P + Pv + A] float64 = dL / d(actor | critic | log_std), written, not accumulated: with dL/dlogp =
 * -w Ahat rho / W on the samples that are not clipped and 0 on the others, g_mu_c = dL/dlogp z_c exp(-ls_c), g_ls_c =
 * sum dL/dlogp (z_c^2 - 1) - ent_coef, g_V = vf_coef w (V - ret) / W, and the two networks' parameter gradients follow
 * from g_mu and g_V as cs_mlp_param_grad forms them from g_actions.  critic_dev NULL: no value term, Pv = 0.
 * stats_dev [8] float64: sum w, L_pi, L_V, H, L, sum w (logp_old - logp) / W, the clipped share of the live samples,
 * max over the live samples of |rho - 1| (0 if there are none).
 *
 * Every sum runs in an order that depends on (B, the widths, the task) alone -- per-workgroup partials added in index
 * order, no floating-point atomics --: equal inputs give equal bits, and index_dev = 0..B-1 gives the bits of index_dev
 * NULL with row_base 0.  clip finite and > 0, vf_coef and ent_coef finite, normalize 0 or 1; obs_dev 16-byte aligned,
 * index_dev, grad_dev and stats_dev 8-byte, every other float pointer 4-byte; with index_dev NULL, 0 <= row_base and
 * row_base + B <= R.  pio->struct_size must be sizeof(cs_ppo_grad_io) (else CS_ERR_ABI); the block is checked before
 * the context and every argument error is raised before any launch.  An open served session is refused.  The first call
 * on a context allocates its scratch (16.5 MB; not under graph capture).  Asynchronous on `stream`; 64-bit offsets. */
typedef struct cs_ppo_grad_io {
  uint32_t struct_size;          /* sizeof(cs_ppo_grad_io) */
  int32_t hidden;                /* the actor's, 0 .. CS_MLP_MAX_HIDDEN */
  int32_t critic_hidden;         /* the critic's, 0 .. CS_MLP_MAX_HIDDEN */
  uint32_t normalize;            /* 0 or 1 */
  int64_t num_rows;              /* R >= 1 */
  int64_t num_samples;           /* B >= 1 */
  int64_t row_base;              /* index_dev NULL: the first row of the minibatch */
  double clip;
  double vf_coef;
  double ent_coef;
  const float* actor_dev;        /* [P] float32, required */
  const float* critic_dev;       /* [Pv] float32, or NULL */
  const float* log_std_dev;      /* [A] float32, required */
  const float* obs_dev;          /* [R,OBS], required */
  const float* actions_dev;      /* [R,A], required */
  const float* logp_dev;         /* [R], required */
  const float* advantages_dev;   /* [R], required */
  const float* returns_dev;      /* [R], required with critic_dev */
  const uint8_t* live_dev;       /* [R], or NULL; a row is live iff its byte is nonzero (2 or 255 count as 1) */
  const int64_t* index_dev;      /* [B], or NULL */
  double* grad_dev;              /* [P + Pv + A], required */
  double* stats_dev;             /* [8], required */
} cs_ppo_grad_io;
int cs_ppo_grad(cs_ctx* ctx, const cs_ppo_grad_io* pio, void* stream);

/* Dynamics.getState() / getStatus() / getTime() (dynamics/__init__.py:199-207, :219-225) for the batch, on
 * the DEVICE and asynchronous (enqueue only, graph-capturable): x_dev [12,N] float32 struct-of-arrays in
 * upstream slot order (the full state, incl. psi / dpsi, which the Lander observation omits),
 * status_dev [N] (CS_STATUS_*), steps_dev [N] (the task's step counter), ticks_dev [N] (Dynamics._ticks;
 * getTime() = ticks * dt; -1 without cfg.track_time).  Each pointer may be NULL. */
int cs_export_state(cs_ctx* ctx, float* x_dev, uint8_t* status_dev, int32_t* steps_dev, int32_t* ticks_dev,
                    void* stream);

/* Whole-batch state exchange with HOST buffers (parity tests, checkpoint/restore): a kernel (de)tiles
 * the state into / from struct-of-arrays staging buffers on the device, and only the arrays asked for
 * cross PCIe.
 * Any pointer may be NULL.  x_host is [12,N] float64 struct-of-arrays in upstream slot
 * order (x,dx,y,dy,z,dz,phi,dphi,theta,dtheta,psi,dpsi); force_xyz_host is [3,N] newtons;
 * flags_host bit0 = perturbation pending, bit1 = reset pending (NEXT_STEP), bit2 = the
 * episode's perturbation is an explicitly installed force rather than the Philox draw of
 * (seed, global env id, episode - 1); force_xyz_host reports that force either way.
 * cs_set_state(force_xyz_host) WITHOUT flags_host installs an explicit force for every env; WITH
 * flags_host it installs one only where bit2 is set and leaves the other envs on their Philox draw,
 * so that cs_set_state(everything cs_get_state returned) is a faithful restore (pending draws keep
 * following cs_seed);
 * prev_shaping NaN = upstream's None; episode_host [N] = episodes started so far per env, a full uint32
 * (episode - 1 is the Philox counter word of the episode's reset draw); ticks_host [N] = Dynamics._ticks
 * (cfg.track_time; -1 / ignored without it). */
int cs_get_state(cs_ctx* ctx, double* x_host, uint8_t* status_host, int32_t* steps_host,
                 double* prev_shaping_host, double* force_xyz_host, uint8_t* flags_host,
                 double* episode_return_host, uint32_t* episode_host, int32_t* ticks_host, void* stream);
int cs_set_state(cs_ctx* ctx, const double* x_host, const uint8_t* status_host,
                 const int32_t* steps_host, const double* prev_shaping_host,
                 const double* force_xyz_host, const uint8_t* flags_host,
                 const double* episode_return_host, const uint32_t* episode_host,
                 const int32_t* ticks_host, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* COPTERSTEP_H */
