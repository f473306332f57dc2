/*
 * qmgpu.h -- C ABI of the MI355X-native MPC + whole-body-control hot path for the AlienGo+Z1
 *            quadruped manipulator (drop-in for the numeric path of danisotelo/qm_door).
 *
 * Nothing like this interface exists in the reference (it has no FFI); each entry point below
 * names the reference interface it replaces (paths relative to the reference tree):
 *
 *   qmgpu_load_problem      <-> qm::QMInterface ctor + setupOptimalControlProblem
 *                               (qm_interface/src/QMInterface.cpp:37-142) and
 *                               WbcBase::loadTasksSetting (qm_wbc/src/WbcBase.cpp:597-627)
 *   qmgpu_create/destroy    <-> QMController::setupMpc / setupWbc
 *                               (qm_controllers/src/QMController.cpp:273-277, 287-307)
 *   qmgpu_mpc_solve_batch   <-> ocs2::MPC_BASE::run -> SqpSolver::runImpl, one SQP iteration
 *                               (object built at qm_controllers/src/QMController.cpp:288-289)
 *   qmgpu_policy_eval_batch <-> MPC_MRT_Interface::evaluatePolicy (QMController.cpp:134-142)
 *   qmgpu_mpc_feedback_batch <-> the LinearController upstream's SqpSolver returns with sqp.useFeedbackPolicy
 *                               (qm_controllers/config/task.info:90; multiple_shooting::remapProjectedGain + toPrimalSolution)
 *   qmgpu_policy_eval_feedback_batch <-> LinearController::computeInput behind MRT_BASE::evaluatePolicy
 *                               (same call site, QMController.cpp:134-142)
 *   qmgpu_warm_start_batch  <-> upstream SqpSolver::runImpl's initial guess from the previous PrimalSolution
 *                               (the solver object built at QMController.cpp:288-289 keeps it between runs)
 *   qmgpu_wbc_solve_batch   <-> qm::WbcBase::update / HierarchicalWbc::update
 *                               (qm_wbc/include/qm_wbc/WbcBase.h:31-34, qm_wbc/src/HierarchicalWbc.cpp:18-44)
 *   qmgpu_cycle_batch       <-> one QMController::update tick fed by one advanceMpc
 *                               (QMController.cpp:129-176, 316-327) for a batch of robots
 *
 * Conventions
 *   - all floating point data is IEEE fp64, all matrices row-major unless stated otherwise
 *   - "dev" pointers are HIP device pointers (HBM resident); the *_host variants take host
 *     pointers and stage through pinned buffers
 *   - the caller owns every buffer; the library owns device scratch behind the opaque handle
 *   - no C++ exception crosses this boundary; every function returns a qmgpu_status
 *   - one handle == one HIP stream; calls on one handle must be serialised by the caller
 *
 * Vector layouts (reference: SURVEY.md Appendix A)
 *   state x[30]   = [ h_lin/m (3), h_ang/m (3) ; p_base (3), yaw, pitch, roll ; q_joint (18) ]
 *   input u[30]   = [ f_LF, f_RF, f_LH, f_RH (12) ; v_joint (18) ]
 *   joints (18)   = LF(HAA,HFE,KFE), LH, RF, RH, z1_joint_1..6          (Pinocchio order)
 *   target[37]    = [ x_ref (30) ; p_ee (3) ; quat_ee (x,y,z,w) ]
 *   rbd[55]       = [ zyx (3), p (3), q_j (18) ; w_world (3), v_lin (3), dq_j (18) ; p_ee (3), quat_ee (4) ]
 *   wbc out[54]   = [ ddq (24), F (12) ; tau (18) ]
 *   mode          = 8*LF + 4*RF + 2*LH + 1*RH   (1 = stance)
 */
#ifndef QMGPU_H
#define QMGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QMGPU_NX 30
#define QMGPU_NU 30
#define QMGPU_NV 24
#define QMGPU_NJ 18
#define QMGPU_NB 19 /* moving bodies: floating base + 18 joint bodies */
#define QMGPU_NC 4  /* 3-DoF contacts, order LF RF LH RH */
#define QMGPU_NTARGET 37
#define QMGPU_NRBD 55
#define QMGPU_NWBC_DEC 36
#define QMGPU_NWBC_OUT 54
#define QMGPU_MAX_EVENTS 40 /* per-instance mode-schedule capacity */
#define QMGPU_NSTATS 10
#define QMGPU_WBC_STATE_WORDS 48 /* uint64 words per instance of qmgpu_wbc_args::working_set */
#define QMGPU_F32_MAX_TARGET_KNOTS 64 /* target knots per instance an fp32 handle (qmgpu_create_ex, QMGPU_F32) can stage; more -> QMGPU_ERR_CAPACITY */

typedef enum qmgpu_status {
  QMGPU_OK = 0,
  QMGPU_ERR_INVALID_ARGUMENT = 1,
  QMGPU_ERR_FILE_NOT_FOUND = 2, /* reference: std::invalid_argument, QMInterface.cpp:45,53,61 */
  QMGPU_ERR_PARSE = 3,
  QMGPU_ERR_UNSUPPORTED_MODEL = 4,
  QMGPU_ERR_NO_DEVICE = 5, /* no HIP device / kernels missing: the library never falls back to a CPU path */
  QMGPU_ERR_HIP = 6,
  QMGPU_ERR_CAPACITY = 7,
  QMGPU_ERR_NUMERICAL = 8
} qmgpu_status;

/* Flat rigid-body model.  Every joint origin of the reference URDF has rpy = 0 and every axis is a
 * positive unit coordinate axis; the loader rejects anything else. */
typedef struct qmgpu_model {
  int32_t parent[QMGPU_NB];          /* parent body, -1 for the base */
  int32_t axis[QMGPU_NB];            /* joint axis 0/1/2 = x/y/z (unused for body 0) */
  double joint_offset[QMGPU_NB][3];  /* joint origin in the parent body frame */
  double mass[QMGPU_NB];             /* fixed children (feet, imu, z1_link_0, gripper) merged in */
  double com[QMGPU_NB][3];           /* body frame */
  double inertia[QMGPU_NB][6];       /* about com, body axes: xx xy xz yy yz zz */
  int32_t foot_body[QMGPU_NC];
  double foot_offset[QMGPU_NC][3];
  int32_t ee_body;
  double ee_offset[3];
  double q_lower[QMGPU_NJ], q_upper[QMGPU_NJ], effort_limit[QMGPU_NJ], velocity_limit[QMGPU_NJ];
  double total_mass;
} qmgpu_model;

typedef struct qmgpu_settings {
  /* model_settings + swing_trajectory_config (task.info:8-31) */
  double position_error_gain, phase_transition_stance_time;
  double liftoff_velocity, touchdown_velocity, swing_height, touchdown_after_horizon, swing_time_scale;
  /* sqp + mpc (task.info:76-93,139-149); alpha_decay/alpha_min/gamma_c/armijo are OCS2 defaults */
  double dt, time_horizon, delta_tol, g_max, g_min, alpha_decay, alpha_min, gamma_c, armijo_factor;
  double cost_tol;                     /* sqp.costTol (upstream default 1e-4): convergence test between SQP iterations */
  int32_t sqp_iterations;
  int32_t use_feedback_policy;         /* sqp.useFeedbackPolicy (task.info:90, default false).  Changes nothing inside the library: a host reads it to decide
                                          whether to call qmgpu_mpc_feedback_batch after a solve (adapters/GpuMpc.h does) */
  /* cost (task.info:193-288) */
  double initial_state[QMGPU_NX];
  double Q[QMGPU_NX * QMGPU_NX];
  double R_task[QMGPU_NU * QMGPU_NU]; /* as loaded; the leg-velocity block is mapped by J^T R J at create time */
  double ee_mu_position, ee_mu_orientation, ee_final_mu_position, ee_final_mu_orientation;
  /* soft constraints (task.info:291-344); cone regularization / hessian shift are OCS2 defaults */
  double friction_coefficient, friction_barrier_mu, friction_barrier_delta, friction_regularization, friction_hessian_shift;
  double joint_pos_barrier_mu, joint_pos_barrier_delta;
  double joint_vel_barrier_mu, joint_vel_barrier_delta;
  double arm_vel_lower[6], arm_vel_upper[6];
  /* reference.info */
  double com_height, default_joint_state[QMGPU_NJ], target_displacement_velocity, target_rotation_velocity;
  /* whole body control (task.info:347-350, qm_wbc/cfg/wbcWigeht.cfg:7-47) */
  double wbc_friction_coefficient;
  double kp_swing, kd_swing, kp_base_height, kd_base_height, kp_base_linear, kd_base_linear, kp_base_angular, kd_base_angular;
  double kp_arm_joint[6], kd_arm_joint[6];
  double kp_ee_linear[3], kd_ee_linear[3], kp_ee_angular[3], kd_ee_angular[3];
  double gravity; /* 9.81 */
  /* Force tracking (BASELINE.json configs[3]; OWN FORMULATION -- the reference's force-tracking branch is not in the mounted tree,
   * README.md:15,161,180 is all it says).  The arm end-effector touches a compliant environment (the door) anchored at p_env(t):
   *     f_e(x, t) = -K_e (p_ee(x) - p_env(t))                              force ON the end-effector, world axes
   * which (1) acts on the centroidal dynamics, d(h_lin)/dt += f_e, d(h_ang)/dt += (p_ee - p_com) x f_e, and (2) is held to a
   * reference by the soft constraint  1/2 mu_f |f_e - f_ref(t)|^2  on the intermediate nodes.  K_e = 0 or a NULL
   * qmgpu_mpc_args::ee_contact_ref switches both off (task.info keys forceTracking.stiffness / forceTracking.muForce). */
  double ee_contact_stiffness, ee_force_mu;
  /* DDP variant (qmgpu_mpc_args::algorithm = QMGPU_ALG_DDP): task.info ddp{} block (:34-72) -- lineSearch.minStepLength / maxStepLength,
   * constraintPenaltyInitialValue */
  double ddp_min_step, ddp_max_step, ddp_constraint_penalty;
} qmgpu_settings;

typedef struct qmgpu_problem {
  qmgpu_model model;
  qmgpu_settings settings;
} qmgpu_problem;

/* A gait template (gait.info) */
typedef struct qmgpu_gait {
  int32_t num_modes;
  int32_t modes[QMGPU_MAX_EVENTS];
  double switching_times[QMGPU_MAX_EVENTS + 1];
} qmgpu_gait;

typedef struct qmgpu_context* qmgpu_handle;

const char* qmgpu_strerror(int status);
/* Last error detail (thread local, valid until the next failing call on this thread). */
const char* qmgpu_last_error(void);

/* ---- host-side configuration (no GPU needed) -------------------------------------------------- */
int qmgpu_load_problem(const char* task_file, const char* urdf_file, const char* reference_file,
                       const char* wbc_gains_file /* may be NULL: compiled-in defaults */, qmgpu_problem* out);
int qmgpu_load_gait(const char* gait_file, const char* gait_name, qmgpu_gait* out);
int qmgpu_mode_from_string(const char* name); /* "LF_RH" -> 9, unknown -> -1 */
/* Tile a gait template over [t_begin, t_end] starting the first cycle at t_phase0, the way
 * ocs2::legged_robot::GaitSchedule extends its template; writes a mode schedule
 * (num_events event times, num_events + 1 modes). Returns QMGPU_ERR_CAPACITY if it does not fit. */
int qmgpu_tile_gait(const qmgpu_gait* gait, double t_phase0, double t_begin, double t_end,
                    int32_t* num_events, double* event_times /*[MAX_EVENTS]*/, int32_t* modes /*[MAX_EVENTS+1]*/);
/* The same for a gait command that arrives while mode `prev_mode` is running (upstream GaitSchedule::insertModeSequenceTemplate behind
 * GaitReceiver, fed by GaitTopicPublisher.cpp:31-44): prev_mode until t_switch; unless prev_mode is STANCE or the template's first mode, a
 * STANCE phase of transition_stance_time (model_settings.phaseTransitionStanceTime, task.info:11) is inserted before the first cycle. */
int qmgpu_switch_gait(const qmgpu_gait* gait, int32_t prev_mode, double transition_stance_time, double t_switch, double t_begin, double t_end,
                      int32_t* num_events, double* event_times /*[MAX_EVENTS]*/, int32_t* modes /*[MAX_EVENTS+1]*/);

/* Shooting grid over [t0, tf] the way upstream ocs2::timeDiscretizationWithEvents lays it out for the SQP solver built at
 * qm_controllers/src/QMController.cpp:288-289 (dt = task.info:79): steps of dt, every event time inside (t0, tf) becomes a
 * node and the dt stepping restarts from it; a remainder shorter than 1e-3 dt is merged into its neighbour.  Upstream keeps a
 * (pre-event, post-event) node pair at the same time; with the identity jump map of this robot the zero-length stage is a
 * no-op and only one node is emitted (a node takes the mode that starts at its time).
 * Writes num_nodes_minus_1 (= N to pass as qmgpu_mpc_args::num_nodes) and grid[0..N].  QMGPU_ERR_CAPACITY if N > max_nodes. */
int qmgpu_time_grid_with_events(double t0, double tf, double dt, int32_t num_events, const double* event_times,
                                int32_t max_nodes, int32_t* num_nodes_minus_1, double* grid);

/* ---- device context ---------------------------------------------------------------------------- */
int qmgpu_create(const qmgpu_problem* problem, int device, int max_batch, int max_nodes, qmgpu_handle* out);
/* Arithmetic type of the MPC kernels behind a handle.  QMGPU_F64 is the reference's (ocs2::scalar_t = double) and what qmgpu_create
 * gives.  QMGPU_F32 runs the whole MPC chain (derivatives, projection, Riccati, line search) in IEEE fp32 on
 * v_mfma_f32_16x16x4_f32 with fp32 scratch; every array of this interface stays fp64 and is converted on the device.  The WBC, the
 * front end and the policy evaluation always run in fp64.  Exists for BASELINE.json configs[4] (fp32-vs-fp64 tolerance sweep,
 * DESIGN.md section 5): fp32 results are NOT within the 1e-6 parity bar of the reference. */
typedef enum qmgpu_dtype { QMGPU_F64 = 0, QMGPU_F32 = 1 } qmgpu_dtype;
int qmgpu_create_ex(const qmgpu_problem* problem, int device, int max_batch, int max_nodes, int dtype, qmgpu_handle* out);
int qmgpu_destroy(qmgpu_handle h);
/* Use an externally owned HIP stream (hipStream_t passed as void*); NULL restores the handle's own stream. */
int qmgpu_set_stream(qmgpu_handle h, void* hip_stream);
int qmgpu_synchronize(qmgpu_handle h);
/* Optional (default off): the WBC launch of qmgpu_cycle_batch goes to a second stream owned by the handle, ordered behind the cycle's policy evaluation.  A WBC launch lasts as
 * long as its slowest instance while most CUs have finished theirs; the node kernels of the NEXT qmgpu_cycle_batch (which do not depend on it -- the reference runs its MPC and
 * its WBC in different threads, QMController.cpp:116-157 / 316-327) then fill those CUs.  With the option on, the WBC outputs of a cycle (out, out_status, input_last, working_set)
 * are complete after qmgpu_synchronize, or on the handle's stream after qmgpu_join_wbc (a device-side wait, no host wait) -- NOT after the caller synchronises its own stream.
 * Which calls join by themselves: qmgpu_cycle_batch (before its policy evaluation), qmgpu_wbc_solve_batch, qmgpu_set_stream (the NEW stream waits), qmgpu_set_overlap,
 * qmgpu_update_settings, qmgpu_debug_poison, qmgpu_synchronize, qmgpu_destroy.  Which do NOT: qmgpu_mpc_solve_batch, qmgpu_policy_eval_batch, qmgpu_mpc_feedback_batch, qmgpu_policy_eval_feedback_batch,
 * qmgpu_mpc_value_function_batch, qmgpu_value_function_eval_batch, qmgpu_mpc_dual_batch, qmgpu_mpc_metrics_batch, qmgpu_mpc_taskspace_batch, qmgpu_frontend_batch, qmgpu_warm_start_batch, qmgpu_gait_schedule_batch, qmgpu_get_input_weight, qmgpu_pack_results -- they touch nothing the library owns that a pending WBC reads or writes, and run next to it.
 * The pending WBC still READS the caller's rbd_measured / period / time (and ee_force) of that cycle and reads and writes input_last / working_set: those buffers must not
 * be modified -- by the caller's own kernels or copies on any stream, or through a non-joining call above -- until qmgpu_join_wbc, qmgpu_synchronize, or the next
 * qmgpu_cycle_batch / qmgpu_wbc_solve_batch has been issued on the handle. */
int qmgpu_set_overlap(qmgpu_handle h, int enable);
int qmgpu_join_wbc(qmgpu_handle h);
/* Replace the settings behind a live handle (gains, weights, limits, barrier parameters; the model is fixed at create time):
 * what the reference's dynamic_reconfigure callbacks do at run time (WbcBase::dynamicCallback, qm_wbc/src/WbcBase.cpp:74-121;
 * QMController::dynamicCallback, qm_controllers/src/QMController.cpp:358-363).  Ordered on the handle's stream: calls enqueued
 * afterwards see the new values; R' is recomputed. */
int qmgpu_update_settings(qmgpu_handle h, const qmgpu_settings* settings);
/* Leg-velocity-mapped input weight R' (30x30, row major) computed at create time (QMInterface.cpp:274-299). */
int qmgpu_get_input_weight(qmgpu_handle h, double* R_host);

/* Per-batch problem data, all device pointers. */
typedef struct qmgpu_mpc_args {
  int32_t batch, num_nodes;            /* N shooting intervals -> N+1 nodes */
  int32_t num_target_knots;            /* K >= 1 */
  int32_t line_search;                 /* 0: take the full step, 1: OCS2 filter line search */
  const double* t0;                    /* [batch] */
  const double* x0;                    /* [batch][30] */
  const double* time_grid;             /* [batch][N+1] or NULL -> t0 + k*dt */
  const double* target_times;          /* [batch][K] */
  const double* target_states;         /* [batch][K][37] */
  const int32_t* sched_num_events;     /* [batch] */
  const double* sched_event_times;     /* [batch][MAX_EVENTS] */
  const int32_t* sched_modes;          /* [batch][MAX_EVENTS+1] */
  const double* warm_x;                /* [batch][N+1][30] or NULL -> initializer (QMInitializer.cpp:33-41) */
  const double* warm_u;                /* [batch][N][30]   or NULL */
  double* out_t;                       /* [batch][N+1] */
  double* out_x;                       /* [batch][N+1][30] */
  double* out_u;                       /* [batch][N][30] */
  int32_t* out_mode;                   /* [batch][N+1] */
  double* out_stats;                   /* [batch][NSTATS]: merit0, violation0, merit1, violation1, alpha, step_type, armijo, status,
                                          SQP iterations performed, convergence (1 iteration limit, 2 step size, 3 metrics, 4 primal step) */
  const double* ee_contact_ref;        /* [batch][K][6] or NULL: per target knot the end-effector force reference f_ref (3) and the anchor
                                          p_env (3) of the compliant environment, interpolated linearly like the other references
                                          (force tracking, see qmgpu_settings::ee_contact_stiffness) */
  int32_t algorithm;                   /* QMGPU_ALG_SQP (0, the solver the reference instantiates) or QMGPU_ALG_DDP */
  int32_t reserved1;
} qmgpu_mpc_args;

/* Solver variants of qmgpu_mpc_solve_batch.
 *   QMGPU_ALG_SQP  multiple-shooting SQP: ocs2::SqpMpc, the object the reference builds (QMController.cpp:288-289, task.info:76-93).
 *   QMGPU_ALG_DDP  single-shooting DDP of the family the task file's ddp{} block configures (task.info:34-72, parsed at QMInterface.cpp:70 but never
 *                  instantiated by the reference): forward rollout of the nonlinear dynamics, LQ approximation along it,
 *                  the same projected Riccati recursion, and a line search that rolls the feedback policy u = u_nom + alpha du_ff + K (x - x_nom) out
 *                  for alpha = maxStepLength * 2^-i >= minStepLength, accepting the first whose merit (cost + constraintPenalty * dt |eq|^2) passes the
 *                  Armijo test.  OWN RESTATEMENT with stated deviations from upstream's SLQ: the rollout uses the shooting grid's RK2 steps (not
 *                  ODE45, task.info:129-137) and the backward pass is the discrete-time recursion (upstream's ILQR form, not the continuous-time
 *                  Riccati ODE).  One iteration per call (ddp.maxNumIterations 1).  The nominal trajectory the LQ approximation is formed along is
 *                  the warm start (warm_x, warm_u) as it is -- a previous solution's defects are part of the linearisation, as in Gauss-Newton
 *                  multiple shooting -- or, without warm_x, the open-loop rollout of warm_u / the initializer's inputs from x0.
 *                  out_stats: merit0, eq-violation0, merit1, eq-violation1, alpha (0 = no step accepted), trials evaluated, armijo, status. */
enum { QMGPU_ALG_SQP = 0, QMGPU_ALG_DDP = 1 };

int qmgpu_mpc_solve_batch(qmgpu_handle h, const qmgpu_mpc_args* args);

/* Linear interpolation of a solved trajectory at t_eval (MRT evaluatePolicy). All device pointers. */
int qmgpu_policy_eval_batch(qmgpu_handle h, int batch, int num_nodes, const double* t_grid, const double* X,
                            const double* U, const int32_t* modes, const double* t_eval, double* x_out /*[batch][30]*/,
                            double* u_out /*[batch][30]*/, int32_t* mode_out /*[batch]*/);

/* The SQP feedback policy.  Replaces the LinearController upstream's SqpSolver returns when sqp.useFeedbackPolicy is set (multiple_shooting::remapProjectedGain,
 * then toPrimalSolution with gains): per node a 30 x 30 gain and a bias such that, near the planned trajectory, the optimal input for a state x at t_k is
 *     u = uff_k + K_k x,        K_k = Px_k + Pu_k K~_k  (row-major; the Riccati gain of the projected problem mapped back to the full input),
 *                               uff_k = U_k - K_k X_k   (so that x = X_k returns the planned input U_k),           k = 0 .. N-1
 *     K_N = K_{N-1},  uff_N = uff_{N-1}                 (upstream repeats the last entry: the arrays are as long as the time grid).
 * X, U: out_x / out_u of the solve (device pointers, as K, uff, status).  K_k is the sensitivity of the first input of the QP over nodes k .. N to its initial
 * state.  Rows 0..11 (contact forces) of a swing foot are zero.
 * Valid after a qmgpu_mpc_solve_batch / qmgpu_cycle_batch with QMGPU_ALG_SQP on the same QMGPU_F64 handle with the same batch and num_nodes; anything else
 * (no solve yet, another shape, a QMGPU_ALG_DDP solve, a QMGPU_F32 handle) returns QMGPU_ERR_INVALID_ARGUMENT.  With sqp.sqpIteration > 1 the gains of an instance
 * belong to the last iteration it performed, the one its out_x / out_u come from.
 * An instance whose solve was flagged (out_stats[7] != 0) gets the feed-forward policy K = 0, uff = U and status[i] != 0; status[i] = 0 otherwise.
 * Enqueued on the handle's stream, no host synchronisation; reads only what the library owns plus X, U.  Does not join a WBC pending on the overlap stream. */
int qmgpu_mpc_feedback_batch(qmgpu_handle h, int batch, int num_nodes, const double* X /*[batch][N+1][30]*/, const double* U /*[batch][N][30]*/,
                             double* K /*[batch][N+1][30][30]*/, double* uff /*[batch][N+1][30]*/, int32_t* status /*[batch] or NULL*/);

/* qmgpu_policy_eval_batch for the feedback policy.  Replaces LinearController::computeInput behind MRT_BASE::evaluatePolicy (QMController.cpp:134-142): uff and K
 * are interpolated linearly at t_eval exactly like U there (same interval, same weight, end values held), then
 *     u_out = uff(t) + K(t) x_measured.
 * x_out and mode_out are bit-identical to qmgpu_policy_eval_batch's.  All device pointers; t_grid / X / modes: out_t / out_x / out_mode of the solve.
 * Intended use: one solve, one qmgpu_mpc_feedback_batch, then per WBC tick qmgpu_policy_eval_feedback_batch with the tick's measured centroidal state (e.g. the x0
 * output of qmgpu_frontend_batch) followed by qmgpu_wbc_solve_batch with state_desired = x_out, input_desired = u_out, mode = mode_out. */
int qmgpu_policy_eval_feedback_batch(qmgpu_handle h, int batch, int num_nodes, const double* t_grid, const double* X, const double* uff /*[batch][N+1][30]*/,
                                     const double* K /*[batch][N+1][30][30]*/, const int32_t* modes, const double* t_eval, const double* x_measured /*[batch][30]*/,
                                     double* x_out /*[batch][30]*/, double* u_out /*[batch][30]*/, int32_t* mode_out /*[batch]*/);

/* The SQP value function.  Replaces SqpSolver::extractValueFunction (sqp.createValueFunction): hpipm getRiccatiCostToGo, re-centred on the linearisation state.
 * For k = 0 .. N, V_k(dx) is the optimal cost of the equality-constrained QP over nodes k .. N of the last SQP iteration the instance performed, as a function of
 * its initial deviation dx_k = dx from the state the instance was linearised at:
 *     Sm_k      Hessian of V_k (row-major, symmetric bit for bit),         sv_lin_k   gradient of V_k at dx = 0,
 *     x_lin_k   the linearisation state (the warm start with row 0 = x0, or x0 at every node for a cold start),
 *     Sv_k = sv_lin_k - Sm_k x_lin_k    (the form upstream stores, so that dfdx(x) = Sv_k + Sm_k x);       Sm_N = sym(Q_N), sv_lin_N = q_N.
 * The constant term is not returned (upstream sets f = 0).  Whether to call is the host's decision: sqp.createValueFunction is not a field of the settings.
 * Valid after a qmgpu_mpc_solve_batch / qmgpu_cycle_batch with QMGPU_ALG_SQP on the same QMGPU_F64 handle with the same batch and num_nodes; anything else
 * (no solve yet, another shape, a QMGPU_ALG_DDP solve, a QMGPU_F32 handle) returns QMGPU_ERR_INVALID_ARGUMENT.  With sqp.sqpIteration > 1 the outputs of an
 * instance belong to the last iteration it performed.  An instance whose solve was flagged (out_stats[7] != 0) gets Sm = 0, Sv = 0, sv_lin = 0, its x_lin, and
 * status[i] != 0; status[i] = 0 otherwise.  All device pointers.  Enqueued on the handle's stream, no host synchronisation; reads only what the library owns and
 * leaves every later solve bit-identical.  Does not join a WBC pending on the overlap stream. */
int qmgpu_mpc_value_function_batch(qmgpu_handle h, int batch, int num_nodes, double* Sm /*[batch][N+1][30][30]*/, double* Sv /*[batch][N+1][30]*/,
                                   double* sv_lin /*[batch][N+1][30] or NULL*/, double* x_lin /*[batch][N+1][30] or NULL*/, int32_t* status /*[batch] or NULL*/);

/* Replaces SqpSolver::getValueFunction(time, state): Sm and Sv are interpolated linearly at t_eval exactly like U in qmgpu_policy_eval_batch (same interval, same
 * weight, end values held), then
 *     dfdxx = Sm(t),      dfdx = Sv(t) + Sm(t) x          (dfdxx symmetric bit for bit; f = 0 upstream, not returned).
 * All device pointers; t_grid: out_t of the solve; Sm, Sv: the outputs of qmgpu_mpc_value_function_batch. */
int qmgpu_value_function_eval_batch(qmgpu_handle h, int batch, int num_nodes, const double* t_grid, const double* Sm /*[batch][N+1][30][30]*/,
                                    const double* Sv /*[batch][N+1][30]*/, const double* t_eval /*[batch]*/, const double* x /*[batch][30]*/,
                                    double* dfdx /*[batch][30]*/, double* dfdxx /*[batch][30][30]*/);

/* The SQP dual solution: what upstream's SqpSolver would hand to getStateInputEqualityConstraintLagrangian / getIntermediateDualSolution.  The multipliers of the
 * equality-constrained QP of the last SQP iteration the instance performed, at its full step (dx, du) (alpha = 1), with the symmetric parts of Q, R:
 *     lambda_N = Q_N dx_N + q_N
 *     lambda_k = Q_k dx_k + q_k + A_k' lambda_{k+1} + C_k' nu_k          k = N-1 .. 0
 *     0        = R_k du_k + r_k + B_k' lambda_{k+1} + D_k' nu_k          k = 0 .. N-1
 *     costate   lambda_k (30 per node): the costate, the gradient of the cost-to-go at the step -- lambda_k = Sm_k dx_k + sv_lin_k of
 *               qmgpu_mpc_value_function_batch, lambda_0 = sv_lin_0 (dx_0 = 0); the multiplier of the dynamics row that ends in node k (of dx_0 = 0 for k = 0),
 *     nu        nu_k: the nc_k <= 16 multipliers of C_k dx + D_k du + e_k = 0 in the row order of qmgpu_debug_get_lq, rows >= nc_k written as zero
 *               (D_k has full row rank: nu_k is unique),
 *     nc        nc_k.
 * Valid after a qmgpu_mpc_solve_batch / qmgpu_cycle_batch with QMGPU_ALG_SQP on the same QMGPU_F64 handle with the same batch and num_nodes; anything else
 * (no solve yet, another shape, a QMGPU_ALG_DDP solve, a QMGPU_F32 handle) returns QMGPU_ERR_INVALID_ARGUMENT.  The costates need only what every solve leaves
 * on the device.  nu also needs the un-projected blocks: a non-NULL nu is valid only if qmgpu_enable_debug(h, 1) was in force during that solve, and returns
 * QMGPU_ERR_INVALID_ARGUMENT otherwise (costate, nc and status alone still work).  With sqp.sqpIteration > 1 the outputs of an instance belong to the last
 * iteration it performed.  An instance whose solve was flagged (out_stats[7] != 0) gets costate = 0, nu = 0, its nc, and status[i] != 0; status[i] = 0 otherwise.
 * All device pointers.  Enqueued on the handle's stream, no host synchronisation; reads only what the library owns and leaves every later solve bit-identical.
 * Does not join a WBC pending on the overlap stream. */
int qmgpu_mpc_dual_batch(qmgpu_handle h, int batch, int num_nodes, double* costate /*[batch][N+1][30]*/, double* nu /*[batch][N][16] or NULL*/,
                         int32_t* nc /*[batch][N] or NULL*/, int32_t* status /*[batch] or NULL*/);

/* The SQP solution metrics: what upstream's SqpSolver::computePerformance forms after every iteration (multiple_shooting::computeIntermediateMetrics /
 * computeTerminalMetrics per node, toPerformanceIndex over the horizon) and SolverBase::getSolutionMetrics / getPerformanceIndeces hand out.  The OCP -- costs, RK2
 * defects, state-input equalities -- evaluated on ANY trajectory (time_grid, X, U): the outputs of a solve, a warm start, a perturbed iterate.
 *     node_cost   Metrics::cost of the node, NOT dt-scaled; entry N the terminal cost.  Bit for bit the left-to-right sum of slots 0..6 of cost_terms.
 *     cost_terms  [0] 1/2 dx'Q dx   [1] 1/2 du'R'du   [2] end-effector pose penalty (ee_mu_*, ee_final_mu_* at node N)   [3] arm joint-position relaxed barrier and
 *                 [4] arm joint-velocity barrier, each with the constant offsets the line search subtracts   [5] friction-cone barrier over the stance feet
 *                 [6] force tracking, exactly 0 with ee_contact_ref == NULL or ee_contact_stiffness == 0   [7] 0.   Terminal node: slot 2 only.
 *     defect      rk2(x_k, u_k, dt_k) - x_{k+1}, dt_k = t_{k+1} - t_k  (Metrics::dynamicsViolation; the b of qmgpu_debug_get_lq at the same point)
 *     eq          values of the state-input equalities in the row order of qmgpu_debug_get_lq's e, rows >= nc_k written as 0 (Metrics::stateInputEqConstraint)
 *     nc          nc_k.  A node takes the contact mode that starts at its time, as the nodes of a solve do: nc equals the solve's for the same grid and schedule.
 *     performance upstream's PerformanceIndex in its field order: [0] merit = cost (this SQP carries no Lagrangian terms)
 *                 [1] cost = sum_{k<N} dt_k node_cost[k] + node_cost[N]   [2] dualFeasibilitiesSSE = 0
 *                 [3] dynamicsViolationSSE = sum dt_k |defect_k|^2 (+ |x0 - X_0|^2 when x0 is given, as upstream counts the initial-state constraint)
 *                 [4] equalityConstraintsSSE = sum dt_k |eq_k|^2   [5] inequalityConstraintsSSE = 0 (every inequality of this OCP is a soft-constraint cost)
 *                 [6] equalityLagrangian = 0   [7] inequalityLagrangian = 0.
 *                 The sums are formed in an order that depends on N only: an instance's eight numbers are the same bits alone and inside a larger batch.
 *                 merit and sqrt([3] + [4]) without x0 are what out_stats[0..1] (at the iterate a solve starts from) and out_stats[2..3] (at out_x / out_u) hold,
 *                 up to the order of summation.
 * Stateless: needs no previous solve, reads the model, the settings and R' behind the handle plus these arrays, writes every entry of every non-NULL output and
 * leaves every later solve bit-identical.  All device pointers.  Enqueued on the handle's stream, no host synchronisation.  QMGPU_F64 handles only; a QMGPU_F32
 * handle, batch / num_nodes beyond the handle's capacity or a missing input return QMGPU_ERR_INVALID_ARGUMENT.  Does not join a WBC pending on the overlap stream.
 * While timing is enabled the call is recorded like a solve; of its six durations only [5], the whole call, is filled. */
enum { QMGPU_NCOST_TERMS = 8, QMGPU_NPERF = 8 };
typedef struct qmgpu_metrics_args {
  int32_t batch, num_nodes, num_target_knots, reserved;
  const double* time_grid;             /* [batch][N+1]  (out_t of a solve, or any increasing grid) */
  const double* X;                     /* [batch][N+1][30] */
  const double* U;                     /* [batch][N][30] */
  const double* x0;                    /* [batch][30] or NULL: adds |x0 - X_0|^2 to the dynamics SSE, as upstream does */
  const double* target_times;          /* as qmgpu_mpc_args */
  const double* target_states;
  const int32_t* sched_num_events;
  const double* sched_event_times;
  const int32_t* sched_modes;
  const double* ee_contact_ref;        /* as qmgpu_mpc_args, may be NULL */
  /* outputs: device pointers, each may be NULL */
  double* node_cost;                   /* [batch][N+1] */
  double* cost_terms;                  /* [batch][N+1][QMGPU_NCOST_TERMS] */
  double* defect;                      /* [batch][N][30] */
  double* eq;                          /* [batch][N][16] */
  int32_t* nc;                         /* [batch][N] */
  double* performance;                 /* [batch][QMGPU_NPERF] */
} qmgpu_metrics_args;
int qmgpu_mpc_metrics_batch(qmgpu_handle h, const qmgpu_metrics_args* args);

/* The planned trajectory in task space: what the consumers next to the solver read off a plan.  Replaces the host-side forward kinematics of upstream's QmVisualizer --
 * publishOptimizedStateTrajectory (qm_interface/src/visualization/qm_visualization.cpp:90-189: the feet, CoM and end-effector lines over every state of the plan, and a
 * "future foothold" wherever a foot lands, :158-181), publishObservation / publishCartesianMarkers (:267-317: foot positions, foot forces, centre of pressure) -- and
 * the host kinematics a caller of qmgpu_frontend_args::feet_height needs.  Evaluated on ANY trajectory (time_grid, X, U): the outputs of a solve, a warm start, a
 * rollout.  Every quantity is an output of the tree sweep the solve differentiates; all vectors are in world axes; foot index c is the contact order of U[3c..3c+2]
 * and of qmgpu_model::foot_body.  With r_c, v_c the position (relative to the base origin) and joint-induced velocity of foot c, r_ee, R_ee the end-effector's, and
 * dp, omega, com_rel the base velocity, angular velocity and centre of mass (relative to the base origin) of the centroidal model at (x_k, u_k):
 *     feet_pos      x_k[6..8] + r_c                                               ee_pos   x_k[6..8] + r_ee
 *     ee_quat       R_ee as a quaternion, x y z w, Eigen's Quaternion(Matrix3) sign rule (ocs2::matrixToQuaternion): the one the end-effector cost compares
 *     com           x_k[6..8] + com_rel
 *     feet_vel      dp + omega x r_c + v_c at (x_k, u_k), k < N: the foot velocity implied by the centroidal momentum and the joint rates -- the three values a stance
 *                   foot contributes to eq of qmgpu_mpc_metrics_batch (with position_error_gain = 0)
 *     base_twist    [dp ; omega], k < N: the base velocity WbcBase::updateDesired reconstructs from the plan (qm_wbc/src/WbcBase.cpp:205-238)
 *     cop           k < N.  With fz_c = u_k[3c+2] and s = ((fz_0 + fz_1) + fz_2) + fz_3, added in this order: (sum_c fz_c feet_pos_c) / s if s > 0, else three zeros.
 *                   The sum runs over all four feet.  This project's own statement of the centre-of-pressure marker upstream draws from the contact forces.
 *     foothold_flag [e][c] = 1 where foot c lands at event e: e < sched_num_events, time_grid[0] < sched_event_times[e] < time_grid[N] (both strict, on the values as
 *                   given), foot c not in contact in sched_modes[e] and in contact in sched_modes[e+1] (qm_visualization.cpp:163-175); 0 everywhere else
 *     foothold_pos  [e][c] the position of foot c at the state interpolated linearly from X at sched_event_times[e] (index and weight of upstream's
 *                   LinearInterpolation::timeSegment, as qmgpu_policy_eval_batch interpolates X) where foothold_flag[e][c] = 1; three zeros everywhere else
 * Stateless: needs no previous solve, reads the model behind the handle plus these arrays, writes every entry of every non-NULL output (events e >= sched_num_events
 * included) and leaves every later solve bit-identical.  An instance's outputs are the same bits alone and inside a larger batch.  All device pointers.  Enqueued on
 * the handle's stream, no host synchronisation.  Does not join a WBC pending on the overlap stream.  Records nothing in the timing ring: qmgpu_last_kernel_ms,
 * qmgpu_kernel_ms_mean and qmgpu_kernel_ms_history are the same before and after it.  QMGPU_ERR_INVALID_ARGUMENT: a QMGPU_F32 handle; batch or num_nodes below 1 or
 * beyond the handle's capacity; time_grid or X missing; feet_vel, base_twist or cop requested with U == NULL; foothold_pos or foothold_flag requested without all three
 * schedule arrays. */
typedef struct qmgpu_taskspace_args {
  int32_t batch, num_nodes;            /* N intervals -> N+1 nodes */
  const double* time_grid;             /* [batch][N+1] */
  const double* X;                     /* [batch][N+1][30] */
  const double* U;                     /* [batch][N][30] or NULL */
  const int32_t* sched_num_events;     /* as qmgpu_mpc_args, or all three NULL */
  const double* sched_event_times;
  const int32_t* sched_modes;
  /* outputs: device pointers, each may be NULL */
  double* feet_pos;                    /* [batch][N+1][4][3] */
  double* ee_pos;                      /* [batch][N+1][3]    */
  double* ee_quat;                     /* [batch][N+1][4]    */
  double* com;                         /* [batch][N+1][3]    */
  double* feet_vel;                    /* [batch][N][4][3]   needs U */
  double* base_twist;                  /* [batch][N][6]      needs U */
  double* cop;                         /* [batch][N][3]      needs U */
  double* foothold_pos;                /* [batch][QMGPU_MAX_EVENTS][4][3]  needs the schedule */
  int32_t* foothold_flag;              /* [batch][QMGPU_MAX_EVENTS][4]     needs the schedule */
} qmgpu_taskspace_args;
int qmgpu_mpc_taskspace_batch(qmgpu_handle h, const qmgpu_taskspace_args* args);

/* Initial guess of the next MPC call from the previous solution: (X, U) of the previous grid resampled (linear interpolation, end values held, as
 * upstream's LinearInterpolation) on new_grid [batch][new_nodes + 1]; x[0] of each instance is overwritten with x0 when x0 != NULL.  The results
 * are what qmgpu_mpc_args::warm_x / warm_u expect.  All device pointers; prev_* and warm_* must not alias. */
int qmgpu_warm_start_batch(qmgpu_handle h, int batch, int prev_nodes, const double* prev_grid, const double* prev_X, const double* prev_U,
                           int new_nodes, const double* new_grid, const double* x0 /*[batch][30] or NULL*/, double* warm_x /*[batch][new_nodes+1][30]*/,
                           double* warm_u /*[batch][new_nodes][30]*/);

typedef struct qmgpu_wbc_args {
  int32_t batch;
  int32_t variant;                     /* 0: HierarchicalWbc, 1: HierarchicalMpcWbc */
  const double* state_desired;         /* [batch][30] */
  const double* input_desired;         /* [batch][30] */
  const double* rbd_measured;          /* [batch][55] */
  const int32_t* mode;                 /* [batch] */
  const double* period;                /* [batch] */
  const double* time;                  /* [batch]  (t < 10 s selects the start-up task set, HierarchicalWbc.cpp:32-37) */
  double* input_last;                  /* [batch][30] in/out: WbcBase::inputLast_ (WbcBase.cpp:224-225) */
  double* out;                         /* [batch][54] */
  int32_t* out_status;                 /* [batch] 0 = all three QPs converged; bit l set = level l hit the iteration cap */
  const double* ee_force;              /* [batch][3] or NULL: external force on the arm end-effector (world axes, measured or from the contact
                                          model); enters the equations of motion, the torque limits and the torque recovery as J_ee^T f_e
                                          (force tracking, own formulation) */
  uint64_t* working_set;               /* [batch][QMGPU_WBC_STATE_WORDS] in/out or NULL: solver state carried from tick to tick, next to input_last.
                                          The reference cold-starts qpOASES on every level of every tick (HoQp.cpp:136-149); consecutive ticks of one
                                          robot end almost always with the same rows on their bounds, so each level's active-set method starts from the
                                          rows the previous tick pinned (same vertex whatever the path; a guess the first step refutes falls back to the
                                          cold path).  Zero-initialise it; zero it again to force a cold tick.
                                          word 0: bit 63 valid | contact mode | variant << 8 | start-up task set << 9  (a tick with another key starts cold)
                                          words 1..12: bit 63 valid | bits 0..55 rows pinned, one word per solve [1 + 6 pass + 2 level + completion]
                                          words 13, 14: passes of every solve of the last tick, pass 0 / canonical pass (one byte per [2 level + completion]:
                                          bits 0..6 interior-point + active-set iterations, bit 7 the carried guess was refuted); word 15 reserved */
} qmgpu_wbc_args;

int qmgpu_wbc_solve_batch(qmgpu_handle h, const qmgpu_wbc_args* args);

/* One control cycle per robot: MPC solve, policy evaluation at t_eval, WBC.  */
int qmgpu_cycle_batch(qmgpu_handle h, const qmgpu_mpc_args* mpc, const double* t_eval /*[batch]*/, qmgpu_wbc_args* wbc);

/* The plant step: the robot the WBC's torques act on.  Advances every instance's 24-DoF rigid-body state -- the model the WBC evaluates -- by dt under a joint
 * command held over the call, with the feet named by `mode` pinned to the ground.
 * THE REFERENCE'S PART is the hybrid joint command law of QMHWSim::writeSim (qm_gazebo/src/QMHWSim.cpp:90-113),
 *     tau_j = kp_j (pos_des_j - q_j) + kd_j (vel_des_j - dq_j) + tau_ff_j        (:112-113, the terms added in this order),
 * with the command QMController::updateControlLaw sets per joint (qm_controllers/src/QMController.cpp:178-191: legs (posDes, velDes, 0, 3, torque) once t > 10 s,
 * arm (posDes, 0, arm_kp_wbc_, arm_kd_wbc_, torque)); tau_ff is the tail out[36..53] of qmgpu_wbc_args::out.  With clamp_effort != 0 the torque is then clamped to
 * the effort limits of the WBC's torque-limit task (the first leg's three limits for every leg, the arm's own).  Not restated: the command delay buffer (:100-111).
 * EVERYTHING ELSE IS THIS PROJECT'S OWN FORMULATION: in the reference this place is taken by the simulator behind QMHWSim.  Coordinates are the WBC's,
 * q = [p, zyx, q_j], v = dq/dt (Euler rates).  The call runs S = substeps steps of h = dt / S; each evaluates the joint law at the current (q, v), then
 *     M(q), nle(q, v) with -J_ee' f_e folded in as the WBC does, Jc(q) = the rows of the feet Jacobian of the feet in contact by `mode`, in foot order,
 *     M (v+ - v) / h + nle = S' tau + Jc' F,     Jc v+ = 0          (velocity-level time stepping, inelastic contacts, F bilateral),
 *     q+ = q + h v+                                                 (semi-implicit Euler; angles are not wrapped),
 * solved by M = L L', Y = L^-1 Jc', G = Y'Y, Cholesky of G (at most 12 x 12; none in flight, mode 0).  Between substeps the state passes through its rbd form, as
 * between calls: S substeps are S calls of dt / S bit for bit, except contact_force and tau_applied, which are the last substep's.  After the last substep rbd_next holds the Euler angles,
 * position and joints of q+, the world angular velocity of the Euler rates (the inverse of the map the WBC applies to rbd_measured), the linear and joint rates,
 * and in slots 48..54 the end-effector position and quaternion (x y z w, the sign rule of qmgpu_taskspace_args::ee_quat) AT q+, as
 * StateEstimateBase::updateArmEE fills them (qm_estimation/src/StateEstimateBase.cpp:89-102).
 *     status  bit 0  a pivot of M or G was not positive, or a result is not finite: rbd_next is the INPUT state, contact_force and tau_applied are zero
 *             bit 1  some stance foot pulls on the ground (F_z < 0) in some substep
 *             bit 2  some stance foot's force lies outside the friction pyramid |F_x|, |F_y| <= mu F_z of settings.wbc_friction_coefficient in some substep
 *             Bits 1 and 2 are reports, not interventions.
 * What this is NOT: contacts come from the schedule, not from geometry; a pinned foot never slips; there is no ground, no penetration and no position-level
 * stabilisation (a pinned foot drifts by O(h^2) per step); no command delay; no joint position limits.
 * Stateless: reads the model and the settings behind the handle plus these arrays, writes every entry of every non-NULL output and leaves every later solve and WBC
 * call bit-identical.  An instance's outputs are the same bits alone and inside a larger batch.  All device pointers; rbd_next may be rbd.  Enqueued on the handle's
 * stream, no host synchronisation.  Does not join a WBC pending on the overlap stream.  Records nothing in the timing ring.  QMGPU_ERR_INVALID_ARGUMENT: a QMGPU_F32
 * handle; batch below 1 or beyond the handle's capacity; substeps < 1; rbd, tau_ff, mode, dt or rbd_next missing; kp without pos_des, kd without vel_des. */
typedef struct qmgpu_plant_args {
  int32_t batch;
  int32_t substeps;                    /* S >= 1: the call advances every robot by S steps of dt / S with the command held */
  int32_t clamp_effort;                /* != 0: the joint torque is clamped to the effort limits the WBC's torque-limit task uses */
  const double* rbd;                   /* [batch][55] state at t (layout of qmgpu_wbc_args::rbd_measured) */
  const double* tau_ff;                /* [batch][18] feed-forward torque (the tail of qmgpu_wbc_args::out) */
  const double* pos_des;               /* [batch][18] or NULL (then kp must be NULL) */
  const double* vel_des;               /* [batch][18] or NULL (then kd must be NULL) */
  const double* kp;                    /* [batch][18] or NULL -> 0 */
  const double* kd;                    /* [batch][18] or NULL -> 0 */
  const int32_t* mode;                 /* [batch] contact mode held during the call, 8 LF + 4 RF + 2 LH + RH */
  const double* dt;                    /* [batch] > 0 */
  const double* ee_force;              /* [batch][3] or NULL: as qmgpu_wbc_args::ee_force */
  double* rbd_next;                    /* [batch][55] state at t + dt; may be the same pointer as rbd */
  double* contact_force;               /* [batch][12] or NULL: F of the LAST substep, world axes, contact order of U[3c..3c+2]; swing feet zero */
  double* tau_applied;                 /* [batch][18] or NULL: joint torque of the last substep after the law and the clamp */
  int32_t* status;                     /* [batch] or NULL */
} qmgpu_plant_args;
int qmgpu_plant_step_batch(qmgpu_handle h, const qmgpu_plant_args* args);

/* The WBC solution report: what a decision vector x = [accelerations (24), contact forces (12)] does to every task of the whole-body controller -- which task is
 * met, which torque or friction limit binds, how far an infeasible limit is exceeded -- and the torque it commands.  An EVALUATOR of any x, not a read-out of
 * the solver: it rebuilds the model terms and the stacked tasks of the tick from the inputs of qmgpu_wbc_args, with the same device functions wbc_kernel runs, and forms
 *     eq_residual[l] = A_l x - b_l     of the stacked equality task of level l = 0, 1, 2 (HierarchicalWbc.cpp:18-44 / HierarchicalMpcWbc.cpp:18-34), rows in the
 *                                      order the builders are stacked, the swing-leg rows of level 1 with their weight of 100; rows >= r_l are zero;
 *     ineq_margin    = f0 - D0 x       of the inequality rows of level 0: rows 0..17 tau_i <= limit_i, rows 18..35 -tau_i <= limit_i (torqueLimits), then five rows
 *                                      of the friction pyramid per stance foot in foot order (-F_z, F_x - mu F_z, -F_x - mu F_z, F_y - mu F_z, -F_y - mu F_z <= 0),
 *                                      then the 3 n_sw all-zero rows frictionCone keeps (margin exactly 0); m_0 = 36 + 5 n_st + 3 n_sw; rows >= m_0 are zero;
 *     tau            = M_j a - J_j' F + nle_j      the torque WbcBase::updateCmd recovers from x (WbcBase.cpp:580-595), with -J_ee' f_e folded into nle as the
 *                                      solve does; margin_i = limit_i - tau_i and margin_{18+i} = limit_i + tau_i;
 *     rows           = r_0, r_1, r_2, m_0;
 *     summary        [0..2] ||A_l x - b_l||_2 per level   [3..5] ||.||_inf per level   [6] minimum margin over the torque rows 0..35
 *                    [7] minimum margin over the friction-pyramid rows, +inf when no foot is in stance
 *                    [8] number of rows i < m_0 with margin_i <= active_tol (1 + |f0_i|)  (on or beyond the limit; the all-zero rows always count)
 *                    [9] number of rows i < m_0 with margin_i < -active_tol (1 + |f0_i|)  (violated)
 *                    [10] index of the row of minimum margin over all m_0 rows (the lowest such index)   [11] reserved, zero.
 *                    Counts and indices are stored as doubles, which is exact.
 * A negative margin is a violated row.  RELATION TO HoQp: the lower levels of the cascade keep the rows of a higher level hard up to the slack that level needed,
 * D x <= f + v (HoQp.cpp:100-124), and hand the slacks on as HoQp::getStackedSlackSolutions (HoQp.h:29, filled at HoQp.cpp:152-158).  The slack is penalised alone
 * (v' v / 2), so at the solution x of the level that owns the rows it is the amount by which a row is exceeded: max(0, -ineq_margin_i) evaluated at that x is the
 * slack HoQp stacks for row i, and at the final x of the cascade max(0, -ineq_margin_i) is at most that slack.  The slacks and working
 * sets as the solver held them are not returned (nothing is read out of wbc_kernel); qmgpu_wbc_report_layout slices the arrays into per-task pieces.
 * input_last is the value inputLast_ had WHEN THE TICK WAS SOLVED: qmgpu_wbc_solve_batch overwrites qmgpu_wbc_args::input_last with input_desired
 * (WbcBase.cpp:224-225), so a caller that wants the report of a solved tick copies input_last before the solve.  The report never writes it.  x is any vector: for a
 * solved tick the head of qmgpu_wbc_args::out (x_stride 54) or a packed copy of it (x_stride 36).
 * Stateless: reads the model and the settings behind the handle plus these arrays, writes every entry of every non-NULL output and leaves every later solve and WBC
 * call bit-identical.  An instance's outputs are the same bits alone and inside a larger batch.  All device pointers.  Enqueued on the handle's stream, no host
 * synchronisation.  Does not join a WBC pending on the overlap stream.  Records nothing in the timing ring.  QMGPU_ERR_INVALID_ARGUMENT: a QMGPU_F32 handle; batch
 * below 1 or beyond the handle's capacity; state_desired, input_desired, rbd_measured, mode, period, time, input_last or x missing; variant outside {0, 1};
 * x_stride outside {36, 54}. */
enum { QMGPU_WBC_REPORT_LEVELS = 3, QMGPU_WBC_REPORT_EQ_ROWS = 22, QMGPU_WBC_REPORT_INEQ_ROWS = 56, QMGPU_WBC_REPORT_SUMMARY = 12 };
typedef struct qmgpu_wbc_report_args {
  int32_t batch;
  int32_t variant;                     /* as qmgpu_wbc_args */
  int32_t x_stride;                    /* doubles between the x of consecutive instances: 36 or 54 */
  int32_t reserved;
  const double* state_desired;         /* [batch][30] */
  const double* input_desired;         /* [batch][30] */
  const double* rbd_measured;          /* [batch][55] */
  const int32_t* mode;                 /* [batch] */
  const double* period;                /* [batch] */
  const double* time;                  /* [batch] */
  const double* ee_force;              /* [batch][3] or NULL */
  const double* input_last;            /* [batch][30] inputLast_ as it was when the tick was solved; read only */
  const double* x;                     /* [batch][x_stride], the first 36 of each read */
  double active_tol;
  /* outputs: device pointers, each may be NULL */
  double* eq_residual;                 /* [batch][3][22] */
  double* ineq_margin;                 /* [batch][56] */
  double* tau;                         /* [batch][18] */
  int32_t* rows;                       /* [batch][4] */
  double* summary;                     /* [batch][12] */
} qmgpu_wbc_report_args;
int qmgpu_wbc_report_batch(qmgpu_handle h, const qmgpu_wbc_report_args* args);

/* The row map of the report (host code, no device): for each of the 13 task builders of WbcBase, named after the reference's methods, where its rows lie.
 * out13[k] describes builder k (its id is k): level -1 when the variant or task set does not use it (first_row and num_rows are then 0), else the level whose
 * stacked task holds it; inequality != 0: its rows lie in ineq_margin, else in eq_residual[level]; first_row / num_rows inside that array (num_rows may be 0: a
 * builder that is stacked with no rows, e.g. swingLeg with four feet in stance); weight: the factor it is stacked with (100 for swingLeg, else 1).
 * frictionCone contributes two pieces: its inequality rows (the pyramid rows of the stance feet followed by the 3 n_sw all-zero rows) under QMGPU_WBC_TASK_FRICTION_CONE
 * and the zero-force equality rows of the swing feet under QMGPU_WBC_TASK_SWING_ZERO_FORCE.  startup != 0 selects the start-up task set (time < 10 s,
 * HierarchicalWbc.cpp:32-37; variant 1 has none).  rows4 (may be NULL) = r_0, r_1, r_2, m_0 as qmgpu_wbc_report_args::rows.  out13 may be NULL.
 * QMGPU_ERR_INVALID_ARGUMENT: variant outside {0, 1}, mode outside 0..15. */
typedef enum qmgpu_wbc_task_id {
  QMGPU_WBC_TASK_FLOATING_BASE_EOM = 0, QMGPU_WBC_TASK_TORQUE_LIMITS = 1, QMGPU_WBC_TASK_NO_CONTACT_MOTION = 2, QMGPU_WBC_TASK_FRICTION_CONE = 3,
  QMGPU_WBC_TASK_BASE_HEIGHT = 4, QMGPU_WBC_TASK_BASE_ANGULAR = 5, QMGPU_WBC_TASK_BASE_LINEAR = 6, QMGPU_WBC_TASK_EE_LINEAR = 7, QMGPU_WBC_TASK_EE_ANGULAR = 8,
  QMGPU_WBC_TASK_SWING_LEG = 9, QMGPU_WBC_TASK_ARM_JOINT_NOMINAL_TRACKING = 10, QMGPU_WBC_TASK_CONTACT_FORCE = 11, QMGPU_WBC_TASK_SWING_ZERO_FORCE = 12,
  QMGPU_WBC_NUM_TASKS = 13
} qmgpu_wbc_task_id;
typedef struct qmgpu_wbc_task_rows {
  int32_t id;                          /* qmgpu_wbc_task_id */
  int32_t level;                       /* 0..2, or -1: not used */
  int32_t inequality;                  /* 0: rows of eq_residual[level]; 1: rows of ineq_margin */
  int32_t first_row;
  int32_t num_rows;
  int32_t reserved;
  double weight;
} qmgpu_wbc_task_rows;
int qmgpu_wbc_report_layout(int variant, int mode, int startup, qmgpu_wbc_task_rows* out13, int32_t* rows4);

/* The solved batch as ONE record per instance, [batch][(N+1)*30 + N*30 + 54 + (N+1)] doubles = X | U | WBC output | contact modes (as doubles: exact): what the ranks of a
 * sharded batch all-gather (the path's only exchange; the collective itself is issued by the host through RCCL).  All device pointers; enqueued
 * on the handle's stream.  Does NOT join a WBC pending on the overlap stream (qmgpu_set_overlap): pack the buffers of a cycle whose WBC has been joined -- behind the
 * next qmgpu_cycle_batch for alternating output buffers, or behind qmgpu_join_wbc. */
int qmgpu_pack_results(qmgpu_handle h, int batch, int num_nodes, const double* X, const double* U, const double* wbc_out, const int32_t* modes, double* packed);

/* ---- front end of a control cycle: what sits immediately before the MPC call ----------
 * (1) state estimate -> MPC observation: rbdState[55] -> centroidal state x[30] with the yaw unwrapped against the previous
 *     observation (QMController::updateStateEstimation, qm_controllers/src/QMController.cpp:239-244; upstream
 *     CentroidalModelRbdConversions::computeCentroidalStateFromRbdModel);
 * (2) command -> TargetTrajectories (two knots of 37-dim states), the free functions of
 *     qm_controllers/src/QmTargetTrajectoriesPublisher_node.cpp:
 *       kind 0  hold           the initial target of QMController::starting (QMController.cpp:107-113)
 *       kind 1  base cmd_vel   cmdVelToTargetTrajectories (:89-129), command = (vx, vy, vz, yaw rate) in the base frame
 *       kind 2  EE cmd_vel     EeCmdVelToTargetTrajectories (:134-188)
 *       kind 3  EE goal pose   EEgoalPoseToTargetTrajectories (:195-238) + positionCommandCallback (:240-254),
 *                              command = position (3) + quaternion x y z w (4)
 * The outputs plug straight into the MPC arguments: x0, target_times, target_states with num_target_knots = 2. */
typedef struct qmgpu_frontend_args {
  int32_t batch;
  const double* rbd_measured;   /* [batch][55] */
  const double* time;           /* [batch] observation time */
  const double* yaw_last;       /* [batch] yaw of the previous observation, or NULL (no unwrapping) */
  const int32_t* command_kind;  /* [batch] 0..3 */
  const double* command;        /* [batch][7] */
  double* last_ee_target;       /* [batch][7] in/out: lastEeTarget_ of the publisher (position + quaternion xyzw) */
  const double* feet_height;    /* [batch] mean z of the contact feet (FEET_HEIGHT, :27-35), or NULL -> 0 */
  double arm_dist;              /* StartingPosition.h:13 (0.6) */
  double start_x, start_y, start_psi; /* StartingPosition.h:9-12 (-2, 0, 0): only kind 0 uses them */
  double* x0;                   /* [batch][30] out */
  double* target_times;         /* [batch][2] out */
  double* target_states;        /* [batch][2][37] out */
} qmgpu_frontend_args;

int qmgpu_frontend_batch(qmgpu_handle h, const qmgpu_frontend_args* args);

/* Gait front end on the device: the per-instance mode schedules of a batch from gait templates, instead of
 * tiling them on the host (qmgpu_tile_gait) and shipping MAX_EVENTS times + modes per instance every cycle.  Replaces, for a batch of
 * robots, what GaitTopicPublisher::gaitCommandCallback (qm_controllers/src/GaitTopicPublisher.cpp:31-44) + upstream GaitReceiver /
 * GaitSchedule::tileModeSequenceTemplate do for one: instance i runs template gait_index[i] of `templates` (host array, copied), first
 * cycle at t_phase0[i] (prev_mode[i] before it -- STANCE when prev_mode is NULL -- with the phase-transition stance of qmgpu_switch_gait,
 * settings.phase_transition_stance_time, where upstream inserts one), tiled over [t_begin[i], t_end[i]], default STANCE after the last tiled
 * cycle.  The outputs are bit-identical to qmgpu_tile_gait / qmgpu_switch_gait and plug straight into qmgpu_mpc_args::sched_*.  status[i] = QMGPU_ERR_CAPACITY (and a pure STANCE
 * schedule) when the schedule needs more than QMGPU_MAX_EVENTS events.  All pointers except `templates` are device pointers. */
int qmgpu_gait_schedule_batch(qmgpu_handle h, int batch, const qmgpu_gait* templates, int num_templates, const int32_t* gait_index,
                              const int32_t* prev_mode /*[batch] or NULL*/, const double* t_phase0 /*[batch]: t_switch of qmgpu_switch_gait*/,
                              const double* t_begin, const double* t_end, int32_t* sched_num_events /*[batch]*/, double* sched_event_times /*[batch][MAX_EVENTS]*/,
                              int32_t* sched_modes /*[batch][MAX_EVENTS+1]*/, int32_t* status /*[batch] or NULL*/);

/* Diagnostics used by the parity tests: per-node LQ blocks of the last qmgpu_mpc_solve_batch
 * (before projection: A B b | Q R q r | C D e ; nc rows valid).  Host pointers, any may be NULL. */
int qmgpu_debug_get_lq(qmgpu_handle h, int instance, int node, double* A, double* B, double* b, double* Q, double* R,
                       double* q, double* r, double* C, double* D, double* e, int32_t* nc);

/* Device time (ms) of each kernel of the last timed call, measured with HIP events on the handle's stream:
 * [0] ad_node  [1] lq_node (projection)  [2] riccati  [3] line search + update  [4] wbc  [5] whole call */
int qmgpu_last_kernel_ms(qmgpu_handle h, double* ms6);
/* Same, averaged over the last `last_calls` timed calls (event ring of 256 calls; no per-call host sync is needed).  Timed qmgpu_mpc_metrics_batch calls in that
 * window are left out of the mean, so that the per-kernel times of the solves stay what they were; a window that holds nothing else returns their mean in [5]. */
int qmgpu_kernel_ms_mean(qmgpu_handle h, int last_calls, double* ms6);
/* The same six durations of EACH of the last `last_calls` timed calls, oldest first: ms6_per_call [last_calls][6] (a launch of the sequential kernels lasts as long as
 * its slowest instance: the spread from call to call is what a real-time caller has to budget for).  A timed qmgpu_mpc_metrics_batch call is one of the calls:
 * its row holds [5] only, [0..4] are 0. */
int qmgpu_kernel_ms_history(qmgpu_handle h, int last_calls, double* ms6_per_call);
int qmgpu_enable_timing(qmgpu_handle h, int enable);
/* Test aid: fills every scratch buffer behind the handle and the LDS of every CU with NaN, so that a kernel reading memory that
 * nothing wrote in this call shows up as NaN in the results instead of passing on left-over values. */
int qmgpu_debug_poison(qmgpu_handle h);
/* Allocate / enable the per-node dump read by qmgpu_debug_get_lq (off by default: 37 KiB per node). */
int qmgpu_enable_debug(qmgpu_handle h, int enable);

#ifdef __cplusplus
}
#endif
#endif /* QMGPU_H */
