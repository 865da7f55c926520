"""ctypes binding of libmpe_hip.so (the C ABI declared in include/mpe_hip.h).

There is no CPU fallback: if the shared object is missing this module raises at import of the
library handle (`lib()`), and every compute entry point needs device pointers.
"""
import ctypes as C
import os

MPE_ABI_VERSION = 4
MPE_MAX_ENTITIES = 512
MPE_ACTION_DIM = 5
MPE_SCN_GENERIC, MPE_SCN_SIMPLE, MPE_SCN_SPREAD, MPE_SCN_TAG, MPE_SCN_ADVERSARY, MPE_SCN_PUSH = 0, 1, 2, 3, 4, 5
MPE_SCN_SPEAKER_LISTENER, MPE_SCN_REFERENCE, MPE_SCN_CRYPTO, MPE_SCN_WORLD_COMM = 6, 7, 8, 9
COMM_KINDS = (MPE_SCN_SPEAKER_LISTENER, MPE_SCN_REFERENCE, MPE_SCN_CRYPTO, MPE_SCN_WORLD_COMM)   # agents speak: MpeBuffers.comm
MPE_MAX_CHOICES = 4
# enum MpeWidePlan: what mpe_wide_plan answers (csrc/mpe_wide.hip's kernels)
MPE_WIDE_NONE, MPE_WIDE_WAVE, MPE_WIDE_MULTI8, MPE_WIDE_MULTI16, MPE_WIDE_MULTI32, MPE_WIDE_DUO, MPE_WIDE_DUO_ROLL = range(7)
# the composable output stage (include/mpe_hip.h, enum MpeRowOp)
MPE_ROWS_MAX_ENTITIES = 64
MPE_ROW_SELF = 255
MPE_ROWS_HEADER_BYTES = 4096
(MPE_ROW_OBS_VEL, MPE_ROW_OBS_POS, MPE_ROW_OBS_REL, MPE_ROW_OBS_REL_PICK, MPE_ROW_OBS_COMM, MPE_ROW_OBS_CONST, MPE_ROW_OBS_ONEHOT,
 MPE_ROW_OBS_REL_VIS, MPE_ROW_OBS_VEL_VIS, MPE_ROW_OBS_IN_REGION) = range(1, 11)
(MPE_ROW_OBS_REL_RANGE, MPE_ROW_OBS_VEL_RANGE, MPE_ROW_OBS_REL_VIS_RANGE, MPE_ROW_OBS_VEL_VIS_RANGE, MPE_ROW_OBS_CONST_N) = range(11, 16)
MPE_ROW_R_MIN_D2_RANGE, MPE_ROW_R_MIN_D2_TO_RANGE, MPE_ROW_R_ADD_IF_HIT_GRID, MPE_ROW_R_ADD_MIN_DIST_GRID = 48, 49, 50, 51
MPE_ROW_R_ABS_POS, MPE_ROW_R_DONE_IF_GT, MPE_ROW_R_DONE_IF_LT, MPE_ROW_R_DONE_IF_HIT = 52, 53, 54, 55
MPE_ROW_OBS_CODE, MPE_ROW_R_CODE, MPE_ROW_R_DONE_CODE = 16, 56, 57      # traced code (symtrace.py): compiled-in programs only
(MPE_ROW_R_D2, MPE_ROW_R_MIN_D2, MPE_ROW_R_D2_PICK, MPE_ROW_R_MIN_D2_PICK, MPE_ROW_R_SQRT, MPE_ROW_R_BOUND, MPE_ROW_R_COMM_ERR,
 MPE_ROW_R_COMM_SUM, MPE_ROW_R_CONST, MPE_ROW_R_SAVE, MPE_ROW_R_LOAD, MPE_ROW_R_ZERO, MPE_ROW_R_ADD, MPE_ROW_R_ADD_IF_HIT,
 MPE_ROW_R_ADD_ACC, MPE_ROW_R_STORE) = range(32, 48)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MPE_HIP_LIB") or os.path.join(_HERE, "lib", "libmpe_hip.so")  # override: A/B builds

_M = MPE_MAX_ENTITIES


class MpeScenarioDesc(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("n_agents", C.c_int32), ("n_landmarks", C.c_int32), ("dim_c", C.c_int32),
        ("n_adversaries", C.c_int32), ("collaborative", C.c_int32),
        ("dt", C.c_float), ("damping", C.c_float), ("contact_force", C.c_float), ("contact_margin", C.c_float),
        ("size", C.c_float * _M), ("mass", C.c_float * _M), ("accel", C.c_float * _M),
        ("max_speed", C.c_float * _M), ("movable", C.c_uint8 * _M), ("collide", C.c_uint8 * _M),
        ("obs_off", C.c_int32 * (_M + 1)),
        ("n_choices", C.c_int32), ("choice_pop", C.c_int32 * MPE_MAX_CHOICES),
    ]


class MpeStepServer(C.Structure):      # include/mpe_hip.h: the step server's device words and ring geometry
    _fields_ = [("door", C.c_void_p), ("flag", C.c_void_p), ("status", C.c_void_p), ("act_ring", C.c_void_p),
                ("ring", C.c_int32), ("slots", C.c_int32), ("timeout_us", C.c_uint64), ("comm_ring", C.c_void_p),
                ("ahead", C.c_int32), ("reserved_", C.c_int32)]


class MpeRenderArgs(C.Structure):      # include/mpe_hip.h: one mpe_render call
    _fields_ = [("pos", C.c_void_p), ("B", C.c_int64), ("worlds", C.c_void_p), ("K", C.c_int32), ("n_entities", C.c_int32),
                ("rgba", C.c_void_p), ("rgba_world_stride", C.c_int32), ("n_viewers", C.c_int32), ("camera", C.POINTER(C.c_int32)),
                ("size", C.c_int32), ("reserved_", C.c_int32), ("out", C.c_void_p)]


MPE_POLICY_MAX_AGENTS, MPE_POLICY_MAX_LAYERS, MPE_POLICY_MAX_WIDTH = 16, 3, 64
MPE_POLICY_MAX_LAUNCH_WORK = 1 << 25      # T * B * A of one mpe_rollout_policy launch
MPE_POLICY_GREEDY, MPE_POLICY_SAMPLE, MPE_POLICY_SOFTMAX = 0, 1, 2
MPE_POLICY_VALUE = 3                     # an MpeActorSet of critics (mpe_critic_q alone accepts it)
MPE_POLICY_RELU, MPE_POLICY_TANH = 0, 1


class MpePolicy(C.Structure):          # include/mpe_hip.h: per-agent MLP actors of mpe_rollout_policy
    _fields_ = [("n_layers", C.c_int32 * MPE_POLICY_MAX_AGENTS), ("width", (C.c_int32 * 4) * MPE_POLICY_MAX_AGENTS),
                ("activation", C.c_int32 * MPE_POLICY_MAX_AGENTS), ("offset", C.c_int64 * MPE_POLICY_MAX_AGENTS),
                ("weights", C.c_void_p), ("mode", C.c_int32), ("reserved_", C.c_int32), ("seed", C.c_uint64)]


MPE_ACTOR_MAX_AGENTS, MPE_ACTOR_MAX_OUT, MPE_ACTOR_MAX_INPUT = 16, 16, 256
MPE_STREAM_POLICY, MPE_STREAM_POLICY_COMM = 0x504F4C49, 0x504F4C43


class MpeActorSet(C.Structure):        # include/mpe_hip.h: the actors of one mpe_actor_act launch
    _fields_ = [("n_agents", C.c_int32), ("mode", C.c_int32), ("seed", C.c_uint64), ("weights", C.c_void_p),
                ("offset", C.c_int64 * MPE_ACTOR_MAX_AGENTS), ("n_layers", C.c_int32 * MPE_ACTOR_MAX_AGENTS),
                ("width", (C.c_int32 * 4) * MPE_ACTOR_MAX_AGENTS), ("activation", C.c_int32 * MPE_ACTOR_MAX_AGENTS),
                ("movable", C.c_uint8 * MPE_ACTOR_MAX_AGENTS), ("speaks", C.c_uint8 * MPE_ACTOR_MAX_AGENTS),
                ("dim_c", C.c_int32), ("reserved_", C.c_int32)]


class MpeTdTarget(C.Structure):        # include/mpe_hip.h: what mpe_critic_q makes the TD target y from
    _fields_ = [("ret", C.c_void_p), ("done", C.c_void_p), ("discount", C.c_void_p), ("gamma", C.c_float), ("reserved_", C.c_int32)]


class MpeGae(C.Structure):             # include/mpe_hip.h: the GAE rule's scalars (mpe_gae)
    _fields_ = [("gamma", C.c_float), ("lambda_", C.c_float), ("episode_len", C.c_int64), ("episode_phase", C.c_int64)]


MPE_STREAM_MINIBATCH = 0x4D494E49


class MpeOnPolicyTraj(C.Structure):    # include/mpe_hip.h: a recorded trajectory as mpe_onpolicy_batch reads it
    _fields_ = [("T", C.c_int64), ("A", C.c_int32), ("dim_c", C.c_int32), ("B", C.c_int64), ("obs_width", C.c_int32 * 16),
                ("obs_in", C.c_void_p), ("act", C.c_void_p), ("utter", C.c_void_p), ("logp", C.c_void_p), ("adv", C.c_void_p),
                ("ret", C.c_void_p), ("val", C.c_void_p)]


MPE_ADAM_MAX_SETS, MPE_ADAM_TILE, MPE_ADAM_MAX_PARTIALS, MPE_ADAM_STATE_DOUBLES = 8, 1024, 256, 16


class MpeAdamSet(C.Structure):         # include/mpe_hip.h: one packed buffer of mpe_adam_step and its gradient and moments
    _fields_ = [("weights", C.c_void_p), ("grad", C.c_void_p), ("m", C.c_void_p), ("v", C.c_void_p), ("n", C.c_int64)]


class MpeAdam(C.Structure):            # include/mpe_hip.h: the scalars and the sets of THE ADAM RULE (mpe_adam_step)
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("weight_decay", C.c_double),
                ("max_grad_norm", C.c_double), ("lr_ptr", C.c_void_p), ("n_sets", C.c_int32), ("reserved_", C.c_int32),
                ("set", MpeAdamSet * MPE_ADAM_MAX_SETS)]


class MpePolicyRows(C.Structure):      # include/mpe_hip.h: the joint row's layout of mpe_policy_rows / mpe_policy_rows_grad
    _fields_ = [("n_agents", C.c_int32), ("W", C.c_int32), ("dim_c", C.c_int32), ("reserved_", C.c_int32), ("col", C.c_int32 * 16),
                ("movable", C.c_uint8 * 16), ("speaks", C.c_uint8 * 16), ("ld", C.c_int64 * 16), ("reg_coef", C.c_double)]


class MpePolyakSet(C.Structure):       # include/mpe_hip.h: one {target, online} pair of packed buffers of mpe_polyak
    _fields_ = [("target", C.c_void_p), ("online", C.c_void_p), ("n", C.c_int64)]


class MpePolyak(C.Structure):          # include/mpe_hip.h: THE POLYAK RULE's tau and pairs (mpe_polyak)
    _fields_ = [("tau", C.c_double), ("tau_ptr", C.c_void_p), ("n_sets", C.c_int32), ("reserved_", C.c_int32),
                ("set", MpePolyakSet * MPE_ADAM_MAX_SETS)]


MPE_Q_INDEPENDENT, MPE_Q_VDN = 0, 1


class MpeQLoss(C.Structure):           # include/mpe_hip.h: the heads and the mix of THE Q LOSS RULE (mpe_q_loss)
    _fields_ = [("n_agents", C.c_int32), ("dim_c", C.c_int32), ("mix", C.c_int32), ("reserved_", C.c_int32),
                ("movable", C.c_uint8 * 16), ("speaks", C.c_uint8 * 16)]


MPE_REPLAY_MAX_AGENTS, MPE_REPLAY_MAX_WIDTH = 16, 4096
MPE_STREAM_REPLAY = 0x5245504C


class MpePpoLoss(C.Structure):         # include/mpe_hip.h: the heads and scalars of THE PPO LOSS RULE (mpe_ppo_loss)
    _fields_ = [("n_agents", C.c_int32), ("dim_c", C.c_int32), ("movable", C.c_uint8 * 16), ("speaks", C.c_uint8 * 16),
                ("clip", C.c_float), ("value_clip", C.c_float), ("vf_coef", C.c_float), ("ent_coef", C.c_float)]


class MpeMlpDinput(C.Structure):       # include/mpe_hip.h: per agent the window of input columns and the row stride of mpe_mlp_dinput's output
    _fields_ = [("col0", C.c_int32 * 16), ("ncol", C.c_int32 * 16), ("ld", C.c_int64 * 16)]


class MpeReplay(C.Structure):          # include/mpe_hip.h: the replay ring of mpe_replay_push / mpe_replay_sample
    _fields_ = [("n_agents", C.c_int32), ("dim_c", C.c_int32), ("B", C.c_int64), ("S", C.c_int64),
                ("obs_width", C.c_int32 * MPE_REPLAY_MAX_AGENTS), ("movable", C.c_uint8 * MPE_REPLAY_MAX_AGENTS),
                ("speaks", C.c_uint8 * MPE_REPLAY_MAX_AGENTS), ("obs", C.c_void_p), ("next_obs", C.c_void_p), ("act", C.c_void_p),
                ("utter", C.c_void_p), ("rew", C.c_void_p), ("done", C.c_void_p), ("head", C.c_void_p), ("ticket", C.c_void_p),
                ("seed", C.c_uint64)]


MPE_REPLAY_MAX_NSTEP = 16


class MpeReplayNStep(C.Structure):     # include/mpe_hip.h: the n-step rule of mpe_replay_sample_nstep / mpe_replay_gather_nstep
    _fields_ = [("n", C.c_int32), ("gamma", C.c_float), ("episode_len", C.c_int64), ("episode_phase", C.c_int64)]


MPE_REPLAY_PRIO_FANOUT, MPE_REPLAY_PRIO_MAX_LEVELS = 16, 11
MPE_REPLAY_PRIO_MIN, MPE_REPLAY_PRIO_MAX = 2.0 ** -40, 2.0 ** 40
MPE_STREAM_REPLAY_PRIO = 0x5250524F


class MpeReplayPrio(C.Structure):      # include/mpe_hip.h: the priorities and their sum tree (mpe_replay_prio_*)
    _fields_ = [("n_leaves", C.c_int64), ("tree", C.c_void_p), ("pmax", C.c_void_p), ("ticket", C.c_void_p)]


class MpeBuffers(C.Structure):
    _fields_ = [
        ("pos", C.c_void_p), ("vel", C.c_void_p), ("act", C.c_void_p), ("ids", C.c_void_p), ("u", C.c_void_p),
        ("obs", C.c_void_p), ("rew", C.c_void_p), ("done", C.c_void_p),
        ("info_rew", C.c_void_p), ("info_collisions", C.c_void_p), ("info_min_dists", C.c_void_p),
        ("info_occupied", C.c_void_p), ("force", C.c_void_p), ("entity_table", C.c_void_p),
        ("comm", C.c_void_p), ("choice", C.c_void_p),
    ]


class MpeRowProgram(C.Structure):
    _fields_ = [
        ("ops_device", C.c_void_p), ("header_device", C.c_void_p), ("header_hash", C.c_uint64), ("n_ops", C.c_int32), ("obs_begin", C.c_int32 * (MPE_ROWS_MAX_ENTITIES + 1)),
        ("rew_begin", C.c_int32 * (MPE_ROWS_MAX_ENTITIES + 1)), ("n_vel", C.c_int32), ("n_regions", C.c_int32),
        ("region_entity", C.c_int32 * 2), ("all_seeing", C.c_uint32), ("image", C.c_void_p),
        ("done_begin", C.c_int32 * (MPE_ROWS_MAX_ENTITIES + 1)), ("reset_boxes", C.c_int32),
        ("reset_box", (C.c_float * 4) * MPE_ROWS_MAX_ENTITIES), ("n_shared", C.c_int32), ("traced", C.c_int32),
    ]


EXPORTS = {
    # name: (restype, argtypes)
    "mpe_abi_version": (C.c_int, []),
    "mpe_last_error": (C.c_char_p, []),
    "mpe_sizeof_desc": (C.c_size_t, []),
    "mpe_sizeof_buffers": (C.c_size_t, []),
    "mpe_fill_obs_layout": (C.c_int, [C.POINTER(MpeScenarioDesc)]),
    "mpe_fill_entity_table": (C.c_int, [C.POINTER(MpeScenarioDesc), C.POINTER(C.c_float)]),
    "mpe_step_supported": (C.c_int, [C.POINTER(MpeScenarioDesc)]),
    "mpe_wide_plan": (C.c_int, [C.POINTER(MpeScenarioDesc), C.POINTER(MpeBuffers), C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                C.POINTER(C.c_int32)]),
    "mpe_step":(C.c_int, [C.POINTER(MpeScenarioDesc), C.POINTER(MpeBuffers), C.c_int64, C.c_void_p]),
    "mpe_step_thread": (C.c_int, [C.POINTER(MpeScenarioDesc), C.POINTER(MpeBuffers), C.c_int64, C.c_void_p]),
    "mpe_observe": (C.c_int, [C.POINTER(MpeScenarioDesc), C.POINTER(MpeBuffers), C.c_int64, C.c_void_p]),
    "mpe_world_step": (C.c_int, [C.POINTER(MpeScenarioDesc), C.POINTER(MpeBuffers), C.c_int64, C.c_void_p]),
    "mpe_apply_action_force": (C.c_int, [C.POINTER(MpeScenarioDesc), C.POINTER(MpeBuffers), C.c_int64, C.c_void_p]),
    "mpe_collision_force": (C.c_int, [C.POINTER(MpeScenarioDesc), C.POINTER(MpeBuffers), C.c_int64, C.c_void_p]),
    "mpe_integrate_state": (C.c_int, [C.POINTER(MpeScenarioDesc), C.POINTER(MpeBuffers), C.c_int64, C.c_void_p]),
    "mpe_reset": (C.c_int, [C.POINTER(MpeScenarioDesc), C.POINTER(MpeBuffers), C.c_int64, C.c_void_p, C.c_float,
                            C.c_uint64, C.c_uint64, C.c_int64, C.c_void_p]),
    "mpe_reset_random_actions_block": (C.c_int, [C.POINTER(MpeScenarioDesc), C.POINTER(MpeBuffers), C.c_int64, C.c_float, C.c_uint64,
                                                 C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int32, C.c_int64, C.c_void_p]),
    "mpe_reset_rows": (C.c_int, [C.POINTER(MpeScenarioDesc), C.POINTER(MpeBuffers), C.POINTER(MpeRowProgram), C.c_int64, C.c_void_p,
                                 C.c_float, C.c_uint64, C.c_uint64, C.c_int64, C.c_void_p]),
    "mpe_random_actions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_uint64,
                                     C.c_int64, C.c_void_p]),
    "mpe_random_actions_block": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_uint64,
                                           C.c_int32, C.c_int64, C.c_void_p]),
    "mpe_random_comm": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_uint32, C.c_uint64, C.c_uint64,
                                  C.c_int32, C.c_int64, C.c_void_p]),
    "mpe_rows_validate": (C.c_int, [C.POINTER(MpeScenarioDesc), C.POINTER(MpeRowProgram), C.POINTER(C.c_int32)]),
    "mpe_rows": (C.c_int, [C.POINTER(MpeScenarioDesc), C.POINTER(MpeBuffers), C.POINTER(MpeRowProgram), C.c_int64, C.c_void_p]),
    "mpe_step_rows": (C.c_int, [C.POINTER(MpeScenarioDesc), C.POINTER(MpeBuffers), C.POINTER(MpeRowProgram), C.c_int64, C.c_void_p]),
    "mpe_episode_finish": (C.c_int, [C.POINTER(MpeScenarioDesc), C.POINTER(MpeBuffers), C.POINTER(MpeRowProgram), C.c_int64, C.c_void_p,
                                     C.c_int32, C.c_float, C.c_uint64, C.c_uint64, C.c_int64, C.c_void_p]),
    "mpe_step_rows_episode": (C.c_int, [C.POINTER(MpeScenarioDesc), C.POINTER(MpeBuffers), C.POINTER(MpeRowProgram), C.c_int64, C.c_void_p,
                                        C.c_int32, C.c_float, C.c_uint64, C.c_uint64, C.c_int64, C.c_void_p]),
    "mpe_rollout_rows": (C.c_int, [C.POINTER(MpeScenarioDesc), C.POINTER(MpeBuffers), C.POINTER(MpeRowProgram), C.c_int64, C.c_int32,
                                   C.c_int32, C.c_float, C.c_uint64, C.c_uint64, C.c_int64, C.c_int32, C.c_uint32, C.c_void_p]),
    "mpe_rollout_rows_episode": (C.c_int, [C.POINTER(MpeScenarioDesc), C.POINTER(MpeBuffers), C.POINTER(MpeRowProgram), C.c_int64, C.c_int32,
                                           C.c_void_p, C.c_int32, C.c_float, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int64, C.c_int32,
                                           C.c_uint32, C.c_void_p]),
    "mpe_sizeof_row_program": (C.c_size_t, []),
    "mpe_sizeof_step_server": (C.c_size_t, []),
    "mpe_rows_static_source": (C.c_int, [C.POINTER(MpeScenarioDesc), C.POINTER(MpeRowProgram), C.POINTER(C.c_int32), C.c_char_p,
                                         C.c_size_t, C.POINTER(C.c_size_t)]),
    "mpe_rows_load_image": (C.c_int, [C.POINTER(MpeScenarioDesc), C.POINTER(MpeRowProgram), C.POINTER(C.c_int32), C.c_void_p,
                                      C.c_size_t]),
    "mpe_rows_unload_image": (C.c_int, [C.POINTER(MpeRowProgram)]),
    "mpe_rows_image_active": (C.c_int, [C.POINTER(MpeScenarioDesc), C.POINTER(MpeRowProgram)]),
    "mpe_episode_tick": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "mpe_rollout_random": (C.c_int, [C.POINTER(MpeScenarioDesc), C.POINTER(MpeBuffers), C.c_int64, C.c_int32,
                                     C.c_int32, C.c_float, C.c_uint64, C.c_uint64, C.c_int64, C.c_int32,
                                     C.c_void_p]),
    "mpe_rollout_actions": (C.c_int, [C.POINTER(MpeScenarioDesc), C.POINTER(MpeBuffers), C.c_int64, C.c_int32, C.c_int32, C.c_float,
                                      C.c_uint64, C.c_uint64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "mpe_rollout_rows_actions": (C.c_int, [C.POINTER(MpeScenarioDesc), C.POINTER(MpeBuffers), C.POINTER(MpeRowProgram), C.c_int64,
                                           C.c_int32, C.c_int32, C.c_float, C.c_uint64, C.c_uint64, C.c_int64, C.c_int32, C.c_void_p,
                                           C.c_void_p]),
    "mpe_step_server_supported": (C.c_int, [C.POINTER(MpeScenarioDesc), C.c_int64]),
    "mpe_step_server_flags": (C.c_int64, [C.c_int64]),
    "mpe_step_server_start": (C.c_int, [C.POINTER(MpeScenarioDesc), C.POINTER(MpeBuffers), C.c_int64, C.c_int32, C.c_int32,
                                        C.c_float, C.c_uint64, C.c_uint64, C.c_int64, C.POINTER(MpeStepServer), C.c_void_p]),
    "mpe_step_server_ring": (C.c_int, [C.POINTER(MpeStepServer), C.c_uint64, C.c_void_p]),
    "mpe_step_server_wait": (C.c_int, [C.POINTER(MpeStepServer), C.c_int64, C.c_uint64, C.c_void_p]),
    "mpe_render": (C.c_int, [C.POINTER(MpeScenarioDesc), C.POINTER(MpeRenderArgs), C.c_void_p]),
    "mpe_sizeof_render_args": (C.c_size_t, []),
    "mpe_sizeof_policy": (C.c_size_t, []),
    "mpe_rollout_policy_supported": (C.c_int, [C.POINTER(MpeScenarioDesc), C.POINTER(MpePolicy), C.c_int64]),
    "mpe_rollout_policy": (C.c_int, [C.POINTER(MpeScenarioDesc), C.POINTER(MpeBuffers), C.POINTER(MpePolicy), C.c_int64, C.c_int32,
                                     C.c_int32, C.c_float, C.c_uint64, C.c_uint64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]),
    "mpe_sizeof_actor_set": (C.c_size_t, []),
    "mpe_actor_supported": (C.c_int, [C.POINTER(MpeActorSet), C.c_int64]),
    "mpe_actor_act": (C.c_int, [C.POINTER(MpeActorSet), C.POINTER(C.c_void_p), C.c_int64, C.c_uint64, C.c_int64, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mpe_actor_act_explore": (C.c_int, [C.POINTER(MpeActorSet), C.POINTER(C.c_void_p), C.c_int64, C.c_uint64, C.c_int64, C.c_double,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mpe_actor_act_rows": (C.c_int, [C.POINTER(MpeActorSet), C.POINTER(C.c_void_p), C.c_int64, C.c_uint64, C.c_int64, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "mpe_sizeof_td_target": (C.c_size_t, []),
    "mpe_critic_q": (C.c_int, [C.POINTER(MpeActorSet), C.POINTER(C.c_void_p), C.c_int64, C.c_void_p, C.POINTER(MpeTdTarget),
                               C.c_void_p, C.c_void_p]),
    "mpe_sizeof_gae": (C.c_size_t, []),
    "mpe_gae_segments": (C.c_int64, [C.c_int64, C.c_int64, C.c_int64]),
    "mpe_gae": (C.c_int, [C.POINTER(MpeGae), C.c_int64, C.c_int32, C.c_int64] + [C.c_void_p] * 7),
    "mpe_sizeof_onpolicy_traj": (C.c_size_t, []),
    "mpe_onpolicy_perm": (C.c_int64, [C.c_int64, C.c_uint64, C.c_uint64, C.c_int64]),
    "mpe_adv_stats_work": (C.c_int64, [C.c_int64, C.c_int32, C.c_int64]),
    "mpe_adv_stats": (C.c_int, [C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mpe_onpolicy_batch": (C.c_int, [C.POINTER(MpeOnPolicyTraj), C.c_int64, C.c_int64, C.c_uint64, C.c_uint64] + [C.c_void_p] * 12),
    "mpe_sizeof_ppo_loss": (C.c_size_t, []),
    "mpe_ppo_loss_work": (C.c_int64, [C.c_int32, C.c_int64]),
    "mpe_ppo_loss": (C.c_int, [C.POINTER(MpePpoLoss), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int64] + [C.c_void_p] * 6 +
                     [C.POINTER(C.c_void_p)] + [C.c_void_p] * 6),
    "mpe_mlp_grad_work": (C.c_int64, [C.POINTER(MpeActorSet), C.c_int64]),
    "mpe_mlp_grad": (C.c_int, [C.POINTER(MpeActorSet), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int64, C.c_void_p, C.c_void_p,
                               C.c_void_p]),
    "mpe_sizeof_mlp_dinput": (C.c_size_t, []),
    "mpe_mlp_dinput": (C.c_int, [C.POINTER(MpeActorSet), C.POINTER(MpeMlpDinput), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int64,
                                 C.POINTER(C.c_void_p), C.c_void_p]),
    "mpe_sizeof_adam": (C.c_size_t, []),
    "mpe_adam_work": (C.c_int64, [C.POINTER(MpeAdam)]),
    "mpe_adam_step": (C.c_int, [C.POINTER(MpeAdam), C.c_void_p, C.c_void_p, C.c_void_p]),
    "mpe_sizeof_policy_rows": (C.c_size_t, []),
    "mpe_sizeof_polyak": (C.c_size_t, []),
    "mpe_td_loss_work": (C.c_int64, [C.c_int32, C.c_int64]),
    "mpe_td_loss": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 6),
    "mpe_policy_rows": (C.c_int, [C.POINTER(MpePolicyRows), C.c_void_p, C.POINTER(C.c_void_p), C.c_int64, C.POINTER(C.c_void_p), C.c_void_p]),
    "mpe_policy_rows_grad_work": (C.c_int64, [C.c_int32, C.c_int64]),
    "mpe_policy_rows_grad": (C.c_int, [C.POINTER(MpePolicyRows), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_int64,
                                       C.POINTER(C.c_void_p)] + [C.c_void_p] * 5),
    "mpe_polyak": (C.c_int, [C.POINTER(MpePolyak), C.c_void_p]),
    "mpe_sizeof_q_loss": (C.c_size_t, []),
    "mpe_q_loss_work": (C.c_int64, [C.c_int32, C.c_int64]),
    "mpe_q_loss": (C.c_int, [C.POINTER(MpeQLoss), C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                             C.POINTER(MpeTdTarget), C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)] + [C.c_void_p] * 7),
    "mpe_sizeof_replay": (C.c_size_t, []),
    "mpe_replay_supported": (C.c_int, [C.POINTER(MpeReplay)]),
    "mpe_replay_push": (C.c_int, [C.POINTER(MpeReplay), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "mpe_replay_sample": (C.c_int, [C.POINTER(MpeReplay), C.c_int64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mpe_replay_gather": (C.c_int, [C.POINTER(MpeReplay), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mpe_sizeof_replay_nstep": (C.c_size_t, []),
    "mpe_replay_sample_nstep": (C.c_int, [C.POINTER(MpeReplay), C.POINTER(MpeReplayNStep), C.c_int64, C.c_uint64] + [C.c_void_p] * 14),
    "mpe_replay_gather_nstep": (C.c_int, [C.POINTER(MpeReplay), C.POINTER(MpeReplayNStep), C.c_int64] + [C.c_void_p] * 14),
    "mpe_sizeof_replay_prio": (C.c_size_t, []),
    "mpe_replay_prio_layout": (C.c_int, [C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mpe_replay_prio_push": (C.c_int, [C.POINTER(MpeReplay), C.POINTER(MpeReplayPrio), C.c_void_p]),
    "mpe_replay_prio_draw": (C.c_int, [C.POINTER(MpeReplay), C.POINTER(MpeReplayPrio), C.c_int64, C.c_uint64, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mpe_replay_prio_update": (C.c_int, [C.POINTER(MpeReplay), C.POINTER(MpeReplayPrio), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mpe_replay_prio_repair": (C.c_int, [C.POINTER(MpeReplay), C.POINTER(MpeReplayPrio), C.c_int64, C.c_int64, C.c_void_p]),
}

_lib = None


class MpeError(RuntimeError):
    pass


def lib():
    """Load libmpe_hip.so once.  torch is imported first so that the HIP runtime already mapped by
    torch (same SONAME libamdhip64.so.7) is the one our kernels register with."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MpeError(
            "%s is missing: build it with `python -m multiagent_particle_envs_amd._build` "
            "(there is no CPU fallback for the step path)" % LIB_PATH)
    import torch  # noqa: F401  (maps torch's libamdhip64 before ours resolves its NEEDED entry)
    handle = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL if hasattr(C, "RTLD_GLOBAL") else 0)
    for name, (res, args) in EXPORTS.items():
        fn = getattr(handle, name)  # AttributeError => symbol not exported
        fn.restype = res
        fn.argtypes = args
    if handle.mpe_abi_version() != MPE_ABI_VERSION:
        raise MpeError("ABI version mismatch: library %d, binding %d" % (handle.mpe_abi_version(), MPE_ABI_VERSION))
    if handle.mpe_sizeof_desc() != C.sizeof(MpeScenarioDesc) or handle.mpe_sizeof_buffers() != C.sizeof(MpeBuffers) or \
            handle.mpe_sizeof_row_program() != C.sizeof(MpeRowProgram) or handle.mpe_sizeof_step_server() != C.sizeof(MpeStepServer) or \
            handle.mpe_sizeof_render_args() != C.sizeof(MpeRenderArgs) or handle.mpe_sizeof_policy() != C.sizeof(MpePolicy) or \
            handle.mpe_sizeof_actor_set() != C.sizeof(MpeActorSet) or handle.mpe_sizeof_replay() != C.sizeof(MpeReplay) or \
            handle.mpe_sizeof_replay_prio() != C.sizeof(MpeReplayPrio) or \
            handle.mpe_sizeof_td_target() != C.sizeof(MpeTdTarget) or \
            handle.mpe_sizeof_gae() != C.sizeof(MpeGae) or \
            handle.mpe_sizeof_onpolicy_traj() != C.sizeof(MpeOnPolicyTraj) or \
            handle.mpe_sizeof_ppo_loss() != C.sizeof(MpePpoLoss) or \
            handle.mpe_sizeof_adam() != C.sizeof(MpeAdam) or \
            handle.mpe_sizeof_mlp_dinput() != C.sizeof(MpeMlpDinput) or \
            handle.mpe_sizeof_q_loss() != C.sizeof(MpeQLoss) or \
            handle.mpe_sizeof_policy_rows() != C.sizeof(MpePolicyRows) or handle.mpe_sizeof_polyak() != C.sizeof(MpePolyak) or \
            handle.mpe_sizeof_replay_nstep() != C.sizeof(MpeReplayNStep):
        raise MpeError("struct layout mismatch between include/mpe_hip.h and _abi.py")
    _lib = handle
    return _lib


def replay_prio_layout(n_leaves):
    """mpe_replay_prio_layout (host only) -> (level offsets off[0..levels], the float count)."""
    levels, off, n = C.c_int32(0), (C.c_int64 * (MPE_REPLAY_PRIO_MAX_LEVELS + 1))(), C.c_int64(0)
    check(lib().mpe_replay_prio_layout(int(n_leaves), C.byref(levels), off, C.byref(n)), "mpe_replay_prio_layout")
    return list(off[:levels.value + 1]), n.value


def wide_plan(desc, bufs, B, phys=True, out=True, roll=False):
    """mpe_wide_plan (host only) -> (MPE_WIDE_* of the kernel such a call launches, homo)."""
    homo = C.c_int32(0)
    plan = lib().mpe_wide_plan(C.byref(desc), C.byref(bufs), int(B), int(phys), int(out), int(roll), C.byref(homo))
    if plan < 0:
        check(plan, "mpe_wide_plan")
    return plan, bool(homo.value)


def raw_stream(device):
    """The current HIP stream of `device` as a ctypes void* (what every entry point takes).  Uses torch's
    raw-handle accessor when it exists: ~0.3 us instead of ~2.5 us for torch.cuda.current_stream(), which
    matters when a step is a 6 us kernel."""
    import torch
    idx = device.index if device.index is not None else torch.cuda.current_device()
    get = getattr(torch._C, "_cuda_getCurrentRawStream", None)
    if get is not None:
        return C.c_void_p(get(idx))
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def check(rc, what=""):
    if rc != 0:
        msg = lib().mpe_last_error().decode("utf-8", "replace")
        raise MpeError("%s failed (code %d): %s" % (what or "libmpe_hip call", rc, msg))
