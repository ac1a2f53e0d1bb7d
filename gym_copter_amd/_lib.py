"""ctypes binding of libcopterstep.so (C ABI declared in include/copterstep.h).

There is deliberately NO fallback: if the shared library is missing or a call fails,
an exception is raised.  Nothing in this package computes environment steps on the CPU.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# COPTERSTEP_LIB selects a diagnostic build of the same ABI (e.g. the stamp build); default = product
LIB_PATH = os.environ.get("COPTERSTEP_LIB", os.path.join(_HERE, "libcopterstep.so"))

ABI_VERSION = 5
TASK_LANDER3D, TASK_HOVER3D, TASK_LANDER2D, TASK_LANDER1D, TASK_HOVER2D, TASK_HOVER1D = range(6)
STATE_F32G, STATE_F32_RN, STATE_F64 = 0, 1, 2
AUTORESET_DISABLED, AUTORESET_NEXT_STEP, AUTORESET_SAME_STEP = 0, 1, 2
STATUS_CRASHED, STATUS_LANDED, STATUS_LEVELING, STATUS_AIRBORNE = 0, 1, 2, 3
ARITH_F64, ARITH_F32 = 0, 1
THRUST_B, THRUST_LIFT = 0, 1
VEHICLE_ROWS = 12
EPISODE_STATS = 7
COMM_ID_BYTES = 128


class CopterStepError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("libcopterstep error %d: %s" % (code, message))
        self.code = code


class Config(C.Structure):
    """Mirror of `struct cs_config` (include/copterstep.h)."""
    _fields_ = [
        ("struct_size", C.c_uint32), ("abi_version", C.c_uint32),
        ("task", C.c_int32), ("state_mode", C.c_int32), ("autoreset", C.c_int32),
        ("substeps", C.c_int32), ("time_limit_truncates", C.c_int32),
        ("episode_stats", C.c_int32), ("device", C.c_int32), ("max_steps", C.c_int32),
        ("num_envs", C.c_int64), ("env_id_base", C.c_int64), ("seed", C.c_uint64),
        ("frames_per_second", C.c_double),
        ("B", C.c_double), ("D", C.c_double), ("M", C.c_double), ("L", C.c_double),
        ("Ix", C.c_double), ("Iy", C.c_double), ("Iz", C.c_double), ("Jr", C.c_double),
        ("maxrpm", C.c_double),
        ("G", C.c_double), ("landing_vel_x", C.c_double), ("landing_vel_y", C.c_double),
        ("landing_angle", C.c_double),
        ("initial_random_force", C.c_double), ("out_of_bounds_penalty", C.c_double),
        ("max_angle_deg", C.c_double), ("bounds", C.c_double), ("initial_altitude", C.c_double),
        ("target_radius", C.c_double), ("yaw_penalty_factor", C.c_double),
        ("xyz_penalty_factor", C.c_double), ("dz_max", C.c_double), ("dz_penalty", C.c_double),
        ("inside_radius_bonus", C.c_double),
        ("action_arith", C.c_int32), ("thrust_model", C.c_int32), ("rotor_gyro", C.c_int32),
        ("track_time", C.c_int32), ("rho", C.c_double), ("C_L", C.c_double),
    ]


class StepIO(C.Structure):
    """Mirror of `struct cs_step_io`."""
    _fields_ = [
        ("actions_dev", C.c_void_p), ("obs_dev", C.c_void_p), ("reward_dev", C.c_void_p),
        ("terminated_dev", C.c_void_p), ("truncated_dev", C.c_void_p),
        ("final_obs_dev", C.c_void_p), ("done_count_dev", C.c_void_p),
        ("done_ids_dev", C.c_void_p), ("done_return_dev", C.c_void_p),
        ("done_length_dev", C.c_void_p), ("output_form", C.c_uint32), ("reserved_", C.c_uint32),
    ]


OUTPUT_AUTO, OUTPUT_PLAIN, OUTPUT_PACKED_ROWS = 0, 1, 2     # cs_step_io.output_form


class JacobianIO(C.Structure):
    """Mirror of `struct cs_jacobian_io` (cs_step_jacobian)."""
    _fields_ = [("struct_size", C.c_uint32), ("out_dtype", C.c_uint32),
                ("actions_dev", C.c_void_p), ("x_dev", C.c_void_p), ("status_dev", C.c_void_p),
                ("force_dev", C.c_void_p), ("dx_dev", C.c_void_p), ("du_dev", C.c_void_p),
                ("reward_dx_dev", C.c_void_p), ("reward_du_dev", C.c_void_p), ("branch_dev", C.c_void_p)]


JAC_F64, JAC_F32 = 0, 1                                      # cs_jacobian_io.out_dtype, cs_rollout_io.out_dtype


class RolloutIO(C.Structure):
    """Mirror of `struct cs_rollout_io` (cs_rollout_states / cs_rollout_vjp)."""
    _fields_ = [("struct_size", C.c_uint32), ("out_dtype", C.c_uint32), ("num_steps", C.c_int32),
                ("reserved_", C.c_uint32), ("actions_dev", C.c_void_p), ("start_x_dev", C.c_void_p),
                ("start_status_dev", C.c_void_p), ("start_force_dev", C.c_void_p),
                ("start_prev_shaping_dev", C.c_void_p), ("x_dev", C.c_void_p), ("reward_dev", C.c_void_p),
                ("terminated_dev", C.c_void_p), ("truncated_dev", C.c_void_p), ("status_dev", C.c_void_p),
                ("gx_dev", C.c_void_p), ("gr_dev", C.c_void_p), ("g_actions_dev", C.c_void_p),
                ("g_x0_dev", C.c_void_p)]


class RolloutParamIO(C.Structure):
    """Mirror of `struct cs_rollout_param_io` (cs_rollout_states_ex / cs_rollout_vjp_ex)."""
    _fields_ = [("struct_size", C.c_uint32), ("out_dtype", C.c_uint32), ("vehicle_dev", C.c_void_p),
                ("g_vehicle_dev", C.c_void_p), ("g_force_dev", C.c_void_p)]


class JvpIO(C.Structure):
    """Mirror of `struct cs_jvp_io` (cs_jvp_rollout)."""
    _fields_ = [("struct_size", C.c_uint32), ("out_dtype", C.c_uint32), ("num_dirs", C.c_int32),
                ("reserved_", C.c_uint32), ("t_actions_dev", C.c_void_p), ("t_x0_dev", C.c_void_p),
                ("t_vehicle_dev", C.c_void_p), ("t_force_dev", C.c_void_p), ("vehicle_dev", C.c_void_p),
                ("t_x_dev", C.c_void_p), ("t_reward_dev", C.c_void_p)]


class RolloutMlpIO(C.Structure):
    """Mirror of `struct cs_rollout_mlp_io` (cs_rollout_mlp_states / cs_rollout_mlp_vjp)."""
    _fields_ = [("struct_size", C.c_uint32), ("hidden", C.c_int32), ("params_dev", C.c_void_p),
                ("offsets_dev", C.c_void_p), ("actions_out_dev", C.c_void_p), ("obs_out_dev", C.c_void_p)]


class RolloutMlpExIO(C.Structure):
    """Mirror of `struct cs_rollout_mlp_ex_io` (cs_rollout_mlp_vjp_ex)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved_", C.c_uint32), ("g_actions_in_dev", C.c_void_p)]


class MlpGradIO(C.Structure):
    """Mirror of `struct cs_mlp_grad_io` (cs_mlp_param_grad)."""
    _fields_ = [("struct_size", C.c_uint32), ("ga_dtype", C.c_uint32), ("hidden", C.c_int32),
                ("num_steps", C.c_int32), ("params_dev", C.c_void_p), ("obs_dev", C.c_void_p),
                ("g_actions_dev", C.c_void_p), ("g_params_dev", C.c_void_p)]


class RolloutLqrIO(C.Structure):
    """Mirror of `struct cs_rollout_lqr_io` (cs_rollout_lqr)."""
    _fields_ = [("struct_size", C.c_uint32), ("out_dtype", C.c_uint32), ("mu", C.c_double),
                ("q_dev", C.c_void_p), ("r_dev", C.c_void_p), ("Q_dev", C.c_void_p), ("Q_final_dev", C.c_void_p),
                ("R_dev", C.c_void_p), ("K_dev", C.c_void_p), ("d_dev", C.c_void_p), ("dV_dev", C.c_void_p),
                ("S0_dev", C.c_void_p), ("s0_dev", C.c_void_p), ("ok_dev", C.c_void_p)]


class RolloutFeedbackIO(C.Structure):
    """Mirror of `struct cs_rollout_feedback_io` (cs_rollout_feedback_states)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved_", C.c_uint32), ("xbar_dev", C.c_void_p),
                ("K_dev", C.c_void_p), ("d_dev", C.c_void_p), ("alpha_dev", C.c_void_p),
                ("actions_out_dev", C.c_void_p)]


class RolloutIlqrBoxIO(C.Structure):
    """Mirror of `struct cs_ilqr_box_io` (cs_ilqr_box_backward / cs_ilqr_box_forward)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved_", C.c_uint32), ("lo_dev", C.c_void_p),
                ("hi_dev", C.c_void_p), ("clamped_dev", C.c_void_p), ("iters_dev", C.c_void_p)]


class RolloutEkfIO(C.Structure):
    """Mirror of `struct cs_rollout_ekf_io` (cs_rollout_ekf)."""
    _fields_ = [("struct_size", C.c_uint32), ("out_dtype", C.c_uint32), ("num_meas", C.c_int32),
                ("reserved_", C.c_uint32), ("H_dev", C.c_void_p), ("r_dev", C.c_void_p), ("Q_dev", C.c_void_p),
                ("P0_dev", C.c_void_p), ("z_dev", C.c_void_p), ("x_pred_dev", C.c_void_p), ("P_dev", C.c_void_p),
                ("P_tape_dev", C.c_void_p), ("var_dev", C.c_void_p), ("nis_dev", C.c_void_p),
                ("loglik_dev", C.c_void_p), ("branch_dev", C.c_void_p), ("ok_dev", C.c_void_p)]


class RolloutLqgIO(C.Structure):
    """Mirror of `struct cs_rollout_lqg_io` (cs_rollout_lqg)."""
    _fields_ = [("struct_size", C.c_uint32), ("out_dtype", C.c_uint32), ("num_meas", C.c_int32),
                ("reserved_", C.c_uint32), ("K_dev", C.c_void_p), ("xbar_dev", C.c_void_p), ("e_dev", C.c_void_p),
                ("H_dev", C.c_void_p), ("r_dev", C.c_void_p), ("Q_dev", C.c_void_p), ("P0_dev", C.c_void_p),
                ("xhat0_dev", C.c_void_p), ("status0_dev", C.c_void_p), ("actions_out_dev", C.c_void_p),
                ("z_dev", C.c_void_p), ("xhat_dev", C.c_void_p), ("x_pred_dev", C.c_void_p), ("P_dev", C.c_void_p),
                ("P_tape_dev", C.c_void_p), ("var_dev", C.c_void_p), ("nis_dev", C.c_void_p),
                ("loglik_dev", C.c_void_p), ("fstatus_dev", C.c_void_p), ("branch_dev", C.c_void_p),
                ("ok_dev", C.c_void_p)]


class RolloutUkfIO(C.Structure):
    """Mirror of `struct cs_rollout_ukf_io` (cs_rollout_ukf)."""
    _fields_ = [("struct_size", C.c_uint32), ("out_dtype", C.c_uint32), ("num_meas", C.c_int32),
                ("reserved_", C.c_uint32), ("gamma", C.c_double), ("wm0", C.c_double), ("wc0", C.c_double),
                ("wi", C.c_double), ("H_dev", C.c_void_p), ("r_dev", C.c_void_p), ("Q_dev", C.c_void_p),
                ("P0_dev", C.c_void_p), ("z_dev", C.c_void_p), ("x_pred_dev", C.c_void_p), ("P_dev", C.c_void_p),
                ("P_tape_dev", C.c_void_p), ("var_dev", C.c_void_p), ("nis_dev", C.c_void_p),
                ("loglik_dev", C.c_void_p), ("spread_dev", C.c_void_p), ("ok_dev", C.c_void_p),
                ("points_dev", C.c_void_p), ("points_pred_dev", C.c_void_p), ("point_status_dev", C.c_void_p)]


class RolloutRtsIO(C.Structure):
    """Mirror of `struct cs_rollout_rts_io` (cs_rollout_rts)."""
    _fields_ = [("struct_size", C.c_uint32), ("out_dtype", C.c_uint32), ("x_f_dev", C.c_void_p),
                ("x_pred_dev", C.c_void_p), ("status_f_dev", C.c_void_p), ("P_f_dev", C.c_void_p),
                ("Q_dev", C.c_void_p), ("P0_dev", C.c_void_p), ("end_x_dev", C.c_void_p), ("end_P_dev", C.c_void_p),
                ("P_tape_dev", C.c_void_p), ("var_dev", C.c_void_p), ("x0_dev", C.c_void_p), ("P0_s_dev", C.c_void_p),
                ("ok_dev", C.c_void_p)]


class RolloutUrtsIO(C.Structure):
    """Mirror of `struct cs_urts_io` (cs_urts_smooth)."""
    _fields_ = [("struct_size", C.c_uint32), ("out_dtype", C.c_uint32), ("gamma", C.c_double), ("wm0", C.c_double),
                ("wc0", C.c_double), ("wi", C.c_double), ("x_f_dev", C.c_void_p), ("x_pred_dev", C.c_void_p),
                ("status_f_dev", C.c_void_p), ("P_f_dev", C.c_void_p), ("Q_dev", C.c_void_p), ("P0_dev", C.c_void_p),
                ("end_x_dev", C.c_void_p), ("end_P_dev", C.c_void_p), ("workspace_dev", C.c_void_p),
                ("P_tape_dev", C.c_void_p), ("var_dev", C.c_void_p), ("x0_dev", C.c_void_p), ("P0_s_dev", C.c_void_p),
                ("ok_dev", C.c_void_p)]


class RolloutPfIO(C.Structure):
    """Mirror of `struct cs_rollout_pf_io` (cs_rollout_pf)."""
    _fields_ = [("struct_size", C.c_uint32), ("out_dtype", C.c_uint32), ("num_meas", C.c_int32),
                ("num_particles", C.c_int32), ("nonce", C.c_uint32), ("first_step", C.c_uint32),
                ("ess_frac", C.c_double), ("H_dev", C.c_void_p), ("r_dev", C.c_void_p), ("Lq_dev", C.c_void_p),
                ("z_dev", C.c_void_p), ("L0_dev", C.c_void_p), ("part_in_dev", C.c_void_p),
                ("pstatus_in_dev", C.c_void_p), ("lw_in_dev", C.c_void_p), ("var_dev", C.c_void_p),
                ("ess_dev", C.c_void_p), ("resampled_dev", C.c_void_p), ("best_dev", C.c_void_p),
                ("P_dev", C.c_void_p), ("loglik_dev", C.c_void_p), ("ok_dev", C.c_void_p),
                ("part_out_dev", C.c_void_p), ("pstatus_out_dev", C.c_void_p), ("lw_out_dev", C.c_void_p),
                ("part_tape_dev", C.c_void_p), ("pstatus_tape_dev", C.c_void_p), ("lw_tape_dev", C.c_void_p),
                ("wq_tape_dev", C.c_void_p), ("anc_tape_dev", C.c_void_p)]


class PfSmoothIO(C.Structure):
    """Mirror of `struct cs_pf_smooth_io` (cs_pf_smooth)."""
    _fields_ = [("struct_size", C.c_uint32), ("out_dtype", C.c_uint32), ("num_particles", C.c_int32),
                ("num_paths", C.c_int32), ("nonce", C.c_uint32), ("first_step", C.c_uint32),
                ("part_tape_dev", C.c_void_p), ("pstatus_tape_dev", C.c_void_p), ("lw_tape_dev", C.c_void_p),
                ("wq_tape_dev", C.c_void_p), ("Linv_dev", C.c_void_p), ("end_idx_dev", C.c_void_p),
                ("part_in_dev", C.c_void_p), ("pstatus_in_dev", C.c_void_p), ("lw_in_dev", C.c_void_p),
                ("idx_dev", C.c_void_p), ("var_dev", C.c_void_p), ("idx0_dev", C.c_void_p), ("ok_dev", C.c_void_p),
                ("logb_tape_dev", C.c_void_p), ("bwq_tape_dev", C.c_void_p)]


class RolloutMppiIO(C.Structure):
    """Mirror of `struct cs_rollout_mppi_io` (cs_rollout_mppi_costs / cs_rollout_mppi_update)."""
    _fields_ = [("struct_size", C.c_uint32), ("num_samples", C.c_int32), ("noise_stream", C.c_uint32),
                ("x_ref_steps", C.c_uint32), ("lam", C.c_double), ("reward_weight", C.c_double),
                ("sigma_dev", C.c_void_p), ("x_ref_dev", C.c_void_p), ("a_ref_dev", C.c_void_p),
                ("Q_dev", C.c_void_p), ("Q_final_dev", C.c_void_p), ("R_dev", C.c_void_p),
                ("costs_dev", C.c_void_p), ("best_dev", C.c_void_p), ("actions_out_dev", C.c_void_p),
                ("ess_dev", C.c_void_p), ("cost_min_dev", C.c_void_p)]


class RolloutMppiExt(C.Structure):
    """Mirror of `struct cs_rollout_mppi_ext` (cs_rollout_mppi_costs_ex / cs_rollout_mppi_update_ex /
    cs_rollout_mppi_temperature)."""
    _fields_ = [("struct_size", C.c_uint32), ("reserved_", C.c_uint32), ("knot_dev", C.c_void_p),
                ("knot_weights_dev", C.c_void_p), ("lam_dev", C.c_void_p), ("ess_target", C.c_double),
                ("lam_min", C.c_double), ("lam_max", C.c_double), ("lam_out_dev", C.c_void_p),
                ("ess_out_dev", C.c_void_p)]


class RolloutPopulationIO(C.Structure):
    """Mirror of `struct cs_rollout_population_io` (cs_rollout_mlp_population)."""
    _fields_ = [("struct_size", C.c_uint32), ("hidden", C.c_int32), ("members", C.c_int32),
                ("envs_per_member", C.c_int32), ("gamma", C.c_double), ("params_table_dev", C.c_void_p),
                ("returns_dev", C.c_void_p), ("lengths_dev", C.c_void_p), ("end_flags_dev", C.c_void_p),
                ("end_status_dev", C.c_void_p), ("member_returns_dev", C.c_void_p)]


class EsIO(C.Structure):
    """Mirror of `struct cs_es_io` (cs_es_perturb / cs_es_gradient)."""
    _fields_ = [("struct_size", C.c_uint32), ("members", C.c_int32), ("num_params", C.c_int32),
                ("noise_stream", C.c_uint32), ("pair_base", C.c_uint32), ("sigma", C.c_float),
                ("params_dev", C.c_void_p), ("table_dev", C.c_void_p), ("weights_dev", C.c_void_p),
                ("grad_dev", C.c_void_p)]


class RolloutAcIO(C.Structure):
    """Mirror of `struct cs_rollout_ac_io` (cs_rollout_actor_critic)."""
    _fields_ = [("struct_size", C.c_uint32), ("num_steps", C.c_int32), ("hidden", C.c_int32),
                ("critic_hidden", C.c_int32), ("nonce", C.c_uint32), ("deterministic", C.c_uint32),
                ("actor_dev", C.c_void_p), ("critic_dev", C.c_void_p), ("log_std_dev", C.c_void_p),
                ("obs_dev", C.c_void_p), ("actions_dev", C.c_void_p), ("means_dev", C.c_void_p),
                ("logp_dev", C.c_void_p), ("values_dev", C.c_void_p), ("reward_dev", C.c_void_p),
                ("flags_dev", C.c_void_p), ("live_dev", C.c_void_p)]


class GaeIO(C.Structure):
    """Mirror of `struct cs_gae_io` (cs_gae)."""
    _fields_ = [("struct_size", C.c_uint32), ("num_steps", C.c_int32), ("flag_stride", C.c_uint32),
                ("reserved_", C.c_uint32), ("gamma", C.c_double), ("lam", C.c_double), ("reward_dev", C.c_void_p),
                ("values_dev", C.c_void_p), ("terminated_dev", C.c_void_p), ("truncated_dev", C.c_void_p),
                ("advantages_dev", C.c_void_p), ("returns_dev", C.c_void_p)]


class PpoGradIO(C.Structure):
    """Mirror of `struct cs_ppo_grad_io` (cs_ppo_grad)."""
    _fields_ = [("struct_size", C.c_uint32), ("hidden", C.c_int32), ("critic_hidden", C.c_int32),
                ("normalize", C.c_uint32), ("num_rows", C.c_int64), ("num_samples", C.c_int64),
                ("row_base", C.c_int64), ("clip", C.c_double), ("vf_coef", C.c_double), ("ent_coef", C.c_double),
                ("actor_dev", C.c_void_p), ("critic_dev", C.c_void_p), ("log_std_dev", C.c_void_p),
                ("obs_dev", C.c_void_p), ("actions_dev", C.c_void_p), ("logp_dev", C.c_void_p),
                ("advantages_dev", C.c_void_p), ("returns_dev", C.c_void_p), ("live_dev", C.c_void_p),
                ("index_dev", C.c_void_p), ("grad_dev", C.c_void_p), ("stats_dev", C.c_void_p)]


ES_PAIR_CHUNK, ES_MAX_MEMBERS, ES_MAX_PARAMS = 32, 65536, 1092   # CS_ES_PAIR_CHUNK, CS_ES_MAX_MEMBERS, CS_ES_MAX_PARAMS
JVP_MAX_DIRS = 64                                            # CS_JVP_MAX_DIRS
URTS_WORKSPACE_ROWS = 102                                    # CS_URTS_WORKSPACE_ROWS
EKF_MAX_MEAS = 12                                            # CS_EKF_MAX_MEAS
PF_MIN_PARTICLES, PF_MAX_PARTICLES = 64, 1024                # CS_PF_MIN_PARTICLES, CS_PF_MAX_PARTICLES
PFS_MAX_PATHS = 1024                                         # CS_PFS_MAX_PATHS
MPPI_MAX_SAMPLES = 65535                                     # CS_MPPI_MAX_SAMPLES
MLP_MAX_HIDDEN = 64                                          # CS_MLP_MAX_HIDDEN
# cs_step_jacobian branch bits (include/copterstep.h: CS_JAC_*)
JAC_INTEGRATED, JAC_LANDED, JAC_CONTACT, JAC_LEVELING, JAC_CRASHED, JAC_RESET, JAC_CLIPPED = 1, 2, 4, 8, 16, 32, 64


# every symbol include/copterstep.h declares: name -> (restype, argtypes)
_P = C.c_void_p
class PidGains(C.Structure):
    """cs_pid_gains (include/copterstep.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("heuristic", C.c_int32)] + \
               [(k, C.c_double) for k in ("rate_kp rate_ki rate_kd rate_windup rate_big_deg pos_kp pos_ki "
                                          "pos_kd pos_target pos_windup descent_kp descent_kd "
                                          "alt_kp alt_ki alt_kd alt_target alt_windup").split()]


class Tuning(C.Structure):
    """cs_tuning (include/copterstep.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("nt_action_max_envs", C.c_uint32),
                ("nt_state_min_envs", C.c_uint32), ("direct_rows_max_envs", C.c_uint32)]


class ServeView(C.Structure):
    """cs_serve_view (include/copterstep.h): the wire description of a served session."""
    _fields_ = [("act_ring", C.c_void_p), ("out_ring", C.c_void_p), ("out_init", C.c_void_p),
                ("ctrl", C.c_void_p), ("spin_limit", C.c_uint64), ("tiles", C.c_uint32), ("ring", C.c_uint32),
                ("act_pieces", C.c_uint32), ("out_pieces", C.c_uint32), ("obs_dim", C.c_uint32),
                ("act_dim", C.c_uint32), ("num_envs", C.c_uint32), ("num_steps", C.c_uint32)]


class LaunchView(C.Structure):
    """cs_launch_view (include/copterstep.h): what a kernel of include/copterstep_rollout.h is launched on."""
    _fields_ = [("struct_size", C.c_uint32), ("abi_version", C.c_uint32), ("consts_size", C.c_uint32),
                ("state_size", C.c_uint32), ("task", C.c_int32), ("state_mode", C.c_int32), ("lean", C.c_int32),
                ("one_call", C.c_int32), ("direct_rows", C.c_int32), ("grid", C.c_uint32), ("block", C.c_uint32),
                ("reserved_", C.c_uint32), ("num_envs", C.c_int64), ("consts", C.c_void_p), ("state", C.c_void_p)]


ERR_ARG, ERR_ABI, ERR_TIMEOUT = -1, -5, -6
PID_LANDER, PID_HOVER = 0, 1
PID_ROWS = 24          # 6 controllers x {errorI, lastError, deltaError1, deltaError2}

SYMBOLS = {
    "cs_version": (C.c_int, []),
    "cs_last_error": (C.c_char_p, []),
    "cs_set_last_error": (None, [C.c_char_p]),
    "cs_config_init": (C.c_int, [C.POINTER(Config), C.c_int]),
    "cs_create": (C.c_int, [C.POINTER(Config), C.POINTER(_P)]),
    "cs_destroy": (C.c_int, [_P]),
    "cs_num_envs": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "cs_obs_dim": (C.c_int, [_P, C.POINTER(C.c_int32)]),
    "cs_action_dim": (C.c_int, [_P, C.POINTER(C.c_int32)]),
    "cs_seed": (C.c_int, [_P, C.c_uint64]),
    "cs_set_altitude": (C.c_int, [_P, C.c_double]),
    "cs_reset": (C.c_int, [_P, _P, _P, _P, _P]),
    "cs_reset_pose": (C.c_int, [_P, _P, _P, C.c_int32, _P, _P, _P]),
    "cs_step": (C.c_int, [_P, _P, _P, _P, _P, _P, _P]),
    "cs_step_ex": (C.c_int, [_P, C.POINTER(StepIO), _P]),
    "cs_step_jacobian": (C.c_int, [_P, C.POINTER(JacobianIO), _P]),
    "cs_rollout_states": (C.c_int, [_P, C.POINTER(RolloutIO), _P]),
    "cs_rollout_vjp": (C.c_int, [_P, C.POINTER(RolloutIO), _P]),
    "cs_rollout_states_ex": (C.c_int, [_P, C.POINTER(RolloutIO), C.POINTER(RolloutParamIO), _P]),
    "cs_rollout_vjp_ex": (C.c_int, [_P, C.POINTER(RolloutIO), C.POINTER(RolloutParamIO), _P]),
    "cs_jvp_rollout": (C.c_int, [_P, C.POINTER(RolloutIO), C.POINTER(JvpIO), _P]),
    "cs_rollout_mlp_states": (C.c_int, [_P, C.POINTER(RolloutIO), C.POINTER(RolloutMlpIO), _P]),
    "cs_rollout_mlp_vjp": (C.c_int, [_P, C.POINTER(RolloutIO), C.POINTER(RolloutMlpIO), _P]),
    "cs_rollout_mlp_vjp_ex": (C.c_int, [_P, C.POINTER(RolloutIO), C.POINTER(RolloutMlpIO), C.POINTER(RolloutMlpExIO),
                                        _P]),
    "cs_mlp_param_grad": (C.c_int, [_P, C.POINTER(MlpGradIO), _P]),
    "cs_rollout_lqr": (C.c_int, [_P, C.POINTER(RolloutIO), C.POINTER(RolloutLqrIO), _P]),
    "cs_rollout_feedback_states": (C.c_int, [_P, C.POINTER(RolloutIO), C.POINTER(RolloutFeedbackIO), _P]),
    "cs_ilqr_box_backward": (C.c_int, [_P, C.POINTER(RolloutIO), C.POINTER(RolloutLqrIO), C.POINTER(RolloutIlqrBoxIO),
                                       _P]),
    "cs_ilqr_box_forward": (C.c_int, [_P, C.POINTER(RolloutIO), C.POINTER(RolloutFeedbackIO),
                                      C.POINTER(RolloutIlqrBoxIO), _P]),
    "cs_rollout_ekf": (C.c_int, [_P, C.POINTER(RolloutIO), C.POINTER(RolloutEkfIO), _P]),
    "cs_rollout_rts": (C.c_int, [_P, C.POINTER(RolloutIO), C.POINTER(RolloutRtsIO), _P]),
    "cs_rollout_pf": (C.c_int, [_P, C.POINTER(RolloutIO), C.POINTER(RolloutPfIO), _P]),
    "cs_rollout_lqg": (C.c_int, [_P, C.POINTER(RolloutIO), C.POINTER(RolloutLqgIO), _P]),
    "cs_rollout_ukf": (C.c_int, [_P, C.POINTER(RolloutIO), C.POINTER(RolloutUkfIO), _P]),
    "cs_urts_smooth": (C.c_int, [_P, C.POINTER(RolloutIO), C.POINTER(RolloutUrtsIO), _P]),
    "cs_pf_smooth": (C.c_int, [_P, C.POINTER(RolloutIO), C.POINTER(PfSmoothIO), _P]),
    "cs_rollout_mppi_costs": (C.c_int, [_P, C.POINTER(RolloutIO), C.POINTER(RolloutMppiIO), _P]),
    "cs_rollout_mppi_update": (C.c_int, [_P, C.POINTER(RolloutIO), C.POINTER(RolloutMppiIO), _P]),
    "cs_rollout_mppi_costs_ex": (C.c_int, [_P, C.POINTER(RolloutIO), C.POINTER(RolloutMppiIO),
                                           C.POINTER(RolloutMppiExt), _P]),
    "cs_rollout_mppi_update_ex": (C.c_int, [_P, C.POINTER(RolloutIO), C.POINTER(RolloutMppiIO),
                                            C.POINTER(RolloutMppiExt), _P]),
    "cs_rollout_mppi_temperature": (C.c_int, [_P, C.POINTER(RolloutMppiIO), C.POINTER(RolloutMppiExt), _P]),
    "cs_rollout_mlp_population": (C.c_int, [_P, C.POINTER(RolloutIO), C.POINTER(RolloutPopulationIO), _P]),
    "cs_es_perturb": (C.c_int, [_P, C.POINTER(EsIO), _P]),
    "cs_es_gradient": (C.c_int, [_P, C.POINTER(EsIO), _P]),
    "cs_rollout_actor_critic": (C.c_int, [_P, C.POINTER(RolloutAcIO), _P]),
    "cs_gae": (C.c_int, [_P, C.POINTER(GaeIO), _P]),
    "cs_ppo_grad": (C.c_int, [_P, C.POINTER(PpoGradIO), _P]),
    "cs_step_many": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "cs_clock_probe": (C.c_int, [_P, C.c_int32, C.POINTER(C.c_double), _P]),
    "cs_device_pci_address": (C.c_int, [_P, C.c_char_p, C.c_int32]),
    "cs_set_motors": (C.c_int, [_P, _P, _P]),
    "cs_set_perturbation": (C.c_int, [_P, _P, _P, _P]),
    "cs_episode_stats": (C.c_int, [_P, _P, _P]),
    "cs_set_tuning": (C.c_int, [_P, C.POINTER(Tuning)]),
    "cs_get_tuning": (C.c_int, [_P, C.POINTER(Tuning)]),
    "cs_comm_unique_id": (C.c_int, [_P]),
    "cs_comm_create": (C.c_int, [_P, C.c_int32, C.c_int32, C.POINTER(_P)]),
    "cs_comm_destroy": (C.c_int, [_P]),
    "cs_allgather": (C.c_int, [_P, _P, _P, C.c_int64, _P]),
    "cs_export_state": (C.c_int, [_P, _P, _P, _P, _P, _P]),
    "cs_set_vehicle_params": (C.c_int, [_P, _P]),
    "cs_pid_gains_init": (C.c_int, [_P]),
    "cs_pid_configure": (C.c_int, [_P, _P]),
    "cs_pid_get_state": (C.c_int, [_P, _P, _P]),
    "cs_pid_set_state": (C.c_int, [_P, _P, _P]),
    "cs_rollout_pid": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "cs_rollout_random": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "cs_get_launch_view": (C.c_int, [_P, _P]),   # for include/copterstep_rollout.h (HIP callers); LaunchView below
    "cs_serve_max_envs": (C.c_int, [_P, C.POINTER(C.c_int64)]),
    "cs_serve_begin": (C.c_int, [_P, C.c_int32, C.c_int32, C.c_double, _P, C.POINTER(ServeView)]),
    "cs_serve_submit": (C.c_int, [_P, C.c_int32, _P, _P]),
    "cs_serve_collect": (C.c_int, [_P, C.c_int32, _P, _P, _P, _P, _P]),
    "cs_serve_policy_pid": (C.c_int, [_P, C.c_int32, _P]),
    "cs_serve_policy_pid_many": (C.c_int, [_P, C.c_int32, C.c_int32, _P]),
    "cs_serve_end": (C.c_int, [_P, _P, C.POINTER(C.c_int32)]),
    "cs_serve_status": (C.c_int, [_P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "cs_get_state": (C.c_int, [_P] + [_P] * 9 + [_P]),
    "cs_set_state": (C.c_int, [_P] + [_P] * 9 + [_P]),
}

_lib = None


def load():
    """Load libcopterstep.so once; raise if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C gym_copter_amd/csrc` (needs hipcc). There is no CPU fallback." % LIB_PATH)
    # PyTorch (used for device memory and streams) bundles its own libamdhip64.so.7.  Import
    # it FIRST so that libcopterstep.so binds to that same, already-loaded HIP runtime by
    # SONAME; loading ours first would put a second HIP/HSA runtime (/opt/rocm) in the
    # process, and the two do not share devices, streams or allocations.
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)      # AttributeError if the symbol is not exported
        fn.restype, fn.argtypes = res, args
    if lib.cs_version() != ABI_VERSION:
        raise ImportError("libcopterstep ABI %d != binding ABI %d" % (lib.cs_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise CopterStepError(rc, load().cs_last_error().decode("utf-8", "replace"))
