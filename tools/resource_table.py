"""One line per kernel from hipcc's -Rpass-analysis=kernel-resource-usage remarks (make report): name | SGPRs | VGPRs |
AGPRs | scratch B/lane | waves/SIMD | LDS B/block, the layout of profiles/*_resources.txt.

    python3 tools/resource_table.py remarks.txt > profiles/rollout_mlp_resources.txt
    python3 tools/resource_table.py remarks.txt mlp_grad > profiles/mlp_grad_resources.txt
    python3 tools/resource_table.py remarks.txt rollout_lqr > profiles/rollout_lqr_resources.txt
    python3 tools/resource_table.py remarks.txt rollout_mppi > profiles/rollout_mppi_resources.txt
    python3 tools/resource_table.py remarks.txt rollout_mppi_smooth > profiles/rollout_mppi_smooth_resources.txt
    python3 tools/resource_table.py remarks.txt rollout_es > profiles/rollout_es_resources.txt
    python3 tools/resource_table.py remarks.txt rollout_ac > profiles/rollout_ac_resources.txt
    python3 tools/resource_table.py remarks.txt ppo_grad > profiles/ppo_grad_resources.txt
    python3 tools/resource_table.py remarks.txt rollout_ekf > profiles/rollout_ekf_resources.txt
    python3 tools/resource_table.py remarks.txt rollout_rts > profiles/rollout_rts_resources.txt
    python3 tools/resource_table.py remarks.txt rollout_pf > profiles/rollout_pf_resources.txt
    python3 tools/resource_table.py remarks.txt rollout_lqg > profiles/rollout_lqg_resources.txt
    python3 tools/resource_table.py remarks.txt rollout_ukf > profiles/rollout_ukf_resources.txt
    python3 tools/resource_table.py remarks.txt ilqr_box > profiles/ilqr_box_resources.txt
    python3 tools/resource_table.py remarks.txt urts > profiles/urts_resources.txt
    python3 tools/resource_table.py remarks.txt rollout_jvp > profiles/rollout_jvp_resources.txt
    python3 tools/resource_table.py remarks.txt pf_smooth > profiles/pf_smooth_resources.txt"""
import re
import sys

FIELDS = (("TotalSGPRs", "SGPRs"), ("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "waves"), ("LDS Size [bytes/block]", "LDS"))


def table(lines):
    rows, cur = [], None
    for line in lines:
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = {"name": re.sub(r"^_ZN2cs12_GLOBAL__N_1\d+", "", m.group(1)).split("EvNS_")[0]}
            rows.append(cur)
            continue
        for key, short in FIELDS:
            m = re.search(r"remark:\s+%s: (\d+)" % re.escape(key), line)
            if m and cur is not None:
                cur[short] = int(m.group(1))
    return rows


HEADS = {"rollout_mlp": """\
# make report (hipcc -Rpass-analysis=kernel-resource-usage), copterstep_rollout_mlp.hip: the closed-loop forward
# rollout_mlp_states_kernel<TASK, MODE> and the backward: rollout_mlp_vjp_kernel<TASK, MODE> (no rotor-gyro term,
# held to 2 wavefronts per SIMD) and rollout_mlp_vjp_gyro_kernel<TASK, MODE>, and the same two with the cotangent on the
# action tape, rollout_mlp_vjp_cot_kernel and rollout_mlp_vjp_gyro_cot_kernel (DESIGN.md section 12).""", "mlp_grad": """\
# make report (hipcc -Rpass-analysis=kernel-resource-usage), copterstep_mlp_grad.hip: the policy-parameter gradient
# mlp_param_grad_kernel<OBS, A, HP> (HP = 0: linear, else the hidden width rounded up to 8, 16, 32 or 64 lanes per row)
# and mlp_grad_sum_kernel, the sum of its workgroups' partials (DESIGN.md section 12).""", "rollout_lqr": """\
# make report (hipcc -Rpass-analysis=kernel-resource-usage), copterstep_rollout_lqr.hip: the iLQR backward pass
# rollout_lqr_kernel<TASK, MODE, GYRO> (its matrices in lane-private LDS columns: one wavefront per CU) and the feedback
# forward rollout_feedback_kernel<TASK, MODE> (DESIGN.md section 13).""", "rollout_mppi": """\
# make report (hipcc -Rpass-analysis=kernel-resource-usage), copterstep_rollout_mppi.hip: the sampled rollouts' costs
# rollout_mppi_costs_kernel<TASK, MODE> (the cost's matrices in 1.3 KiB of LDS), the arg-min mppi_best_kernel and the
# weighted update rollout_mppi_update_kernel<TASK> (DESIGN.md section 14).""", "rollout_mppi_smooth": """\
# make report (hipcc -Rpass-analysis=kernel-resource-usage), copterstep_rollout_mppi_smooth.hip: the costs under knot
# noise rollout_mppi_smooth_costs_kernel<TASK, MODE> (the cost's matrices and the two knot draws of the A components,
# a lane-private column each, in the LDS: the draws do not fit the registers of the 3D tasks without scratch), the
# arg-min mppi_best_kernel, the update rollout_mppi_smooth_update_kernel<TASK> with its per-env temperature and the
# bisection mppi_temperature_kernel (DESIGN.md section 15).""", "rollout_es": """\
# make report (hipcc -Rpass-analysis=kernel-resource-usage), copterstep_rollout_es.hip: the population rollout
# rollout_mlp_population_kernel<TASK, MODE> (each wavefront under its member's weights, read by scalar loads; no LDS; 3 wavefronts per SIMD),
# the member mean member_mean_kernel, the mirrored population es_perturb_kernel and the search gradient
# es_gradient_kernel with its fixed-order sum es_gradient_sum_kernel (DESIGN.md section 16).""", "rollout_ac": """\
# make report (hipcc -Rpass-analysis=kernel-resource-usage), copterstep_rollout_ac.hip: the actor-critic collection
# rollout_ac_kernel<TASK, MODE> (both networks' weights read by scalar loads; no LDS) and the advantages gae_kernel
# (DESIGN.md section 17).""", "ppo_grad": """\
# make report (hipcc -Rpass-analysis=kernel-resource-usage), copterstep_ppo_grad.hip: PPO's minibatch loss and gradient
# ppo_grad_kernel<OBS, A, HP, HEAD> (HP = 0: linear, else the hidden width rounded up to 8, 16, 32 or 64 lanes per row;
# HEAD 0 = the Gaussian policy, 1 = the value function), the two passes over the advantages ppo_adv_kernel<PASS> and
# ppo_grad_sum_kernel, the sum of the workgroups' partials and the statistics (DESIGN.md section 18).""", "rollout_ekf": """\
# make report (hipcc -Rpass-analysis=kernel-resource-usage), copterstep_rollout_ekf.hip: the extended Kalman filter
# rollout_ekf_kernel<TASK, MODE, GYRO> (the covariance, W = A P and the means in lane-private LDS columns: one wavefront
# per CU; DESIGN.md section 19).""", "rollout_rts": """\
# make report (hipcc -Rpass-analysis=kernel-resource-usage), copterstep_rollout_rts.hip: the Rauch-Tung-Striebel smoother
# rollout_rts_kernel<TASK, MODE, GYRO> (two packed covariances, W = A P / the gain and the smoothed mean in lane-private
# LDS columns: one wavefront per CU; DESIGN.md section 20).""", "rollout_pf": """\
# make report (hipcc -Rpass-analysis=kernel-resource-usage), copterstep_rollout_pf.hip: the bootstrap particle filter
# rollout_pf_kernel<TASK, MODE, GYRO> (one workgroup of min(P, 256) lanes per env; the particles, their weights and the
# cumulative weights in dynamic LDS, 124 P + 3 072 bytes per workgroup -- not part of the static figure below; DESIGN.md
# section 21).""", "rollout_lqg": """\
# make report (hipcc -Rpass-analysis=kernel-resource-usage), copterstep_rollout_lqg.hip: the output-feedback rollout
# rollout_lqg_kernel<TASK, MODE, GYRO> (the filter's covariance, W = A P and means and the parked true state in
# lane-private LDS columns, 265 rows: one wavefront per CU; DESIGN.md section 22).""", "rollout_ukf": """\
# make report (hipcc -Rpass-analysis=kernel-resource-usage), copterstep_rollout_ukf.hip: the unscented Kalman filter
# rollout_ukf_kernel<TASK, MODE, GYRO> (the covariance, its factor, the moment sum, the mean and the propagated centre
# point in lane-private LDS columns, 258 rows: one wavefront per CU; DESIGN.md section 23).""", "ilqr_box": """\
# make report (hipcc -Rpass-analysis=kernel-resource-usage), copterstep_ilqr_box.hip: the control-limited iLQR backward
# ilqr_box_backward_kernel<TASK, MODE, GYRO> (rollout_lqr_kernel's LDS rows, not one more: the box-constrained programme
# of each step runs in registers) and the clamped feedback forward ilqr_box_forward_kernel<TASK, MODE> (DESIGN.md
# section 24).""", "urts": """\
# make report (hipcc -Rpass-analysis=kernel-resource-usage), copterstep_urts.hip: the unscented Rauch-Tung-Striebel
# smoother urts_kernel<TASK, MODE, GYRO> (the factor, the moment sum, the cross-covariance / gain and the propagated
# centre point in lane-private LDS columns, 313 rows: one wavefront per CU; the smoothed row above is parked in the
# caller's workspace while the points run; DESIGN.md section 25).""", "rollout_jvp": """\
# make report (hipcc -Rpass-analysis=kernel-resource-usage), copterstep_jvp.hip: the forward-mode rollout tangents
# rollout_jvp_kernel<TASK, MODE, GYRO, PARAM> (6 KiB of LDS for the tangent rows; PARAM builds keep the direction
# block's 2 x 11 coefficient tangents in lane-private LDS columns, 11 KiB more; DESIGN.md section 26).""", "pf_smooth": """\
# make report (hipcc -Rpass-analysis=kernel-resource-usage), copterstep_pf_smooth.hip: the backward-simulation particle
# smoother pf_smooth_kernel<TASK, MODE, GYRO> (one workgroup of min(P, 256) lanes per env; the whitened particles, their
# log-weights and statuses and two rows of path indices in dynamic LDS, 108 P + 16 656 bytes per workgroup -- not part
# of the static figure below; DESIGN.md section 27)."""}


def main(path, which="rollout_mlp"):
    rows = table(open(path).read().splitlines())
    print(HEADS[which])
    print("# Name | SGPRs | VGPRs | AGPRs | scratch B/lane | waves/SIMD | LDS B/block")
    for r in rows:
        print("|".join([r["name"]] + [str(r.get(s, "?")) for _, s in FIELDS]))
    spill = [r["name"] for r in rows if r.get("scratch", 0) != 0]
    print("# %d kernels; scratch in %d of them" % (len(rows), len(spill)))
    return 1 if spill else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
