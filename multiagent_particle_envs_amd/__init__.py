"""MI355X-native batched multi-agent particle environment: the `MultiAgentEnv.step` hot path of
openai/multiagent-particle-envs as hand-written HIP kernels (gfx950) behind a C ABI, driven from
Python with PyTorch-ROCm tensors holding the SoA world state.  See DESIGN.md."""
from .make_env import make_env  # noqa: F401
from .environment import MultiAgentEnv, BatchMultiAgentEnv, GraphedStep  # noqa: F401
from .scenario import BaseScenario  # noqa: F401
from . import core, scenarios  # noqa: F401
from .rollout import MlpPolicy, PolicyRollout, PolicyTrajectory  # noqa: F401
from .policy import Actors, PolicyLoop  # noqa: F401
from .learner import Critics, TdTargets  # noqa: F401
from .learner import (TdLoss, TdLossResult, td_loss_tensors, ActorLoss, RowsLayout, PolicyRowsGradResult,  # noqa: F401
                      policy_rows_tensors, policy_rows_grad_tensors)
from .learner import QLoss, QLossResult, QTargets, q_loss_tensors  # noqa: F401
from .onpolicy import Values, GaeResult, gae, gae_tensors, adv_stats, Minibatches, OnPolicyBatch  # noqa: F401
from .onpolicy import PpoLoss, PpoLossResult, ppo_loss_tensors  # noqa: F401
from .train import Trainable, MlpGradResult, mlp_grad_tensors, mlp_dinput_tensors  # noqa: F401
from .optim import DeviceAdam, PolyakTargets  # noqa: F401
from .replay import (ReplayBuffer, ReplayBatch, NStepReplayBatch, PrioritizedReplayBuffer, PrioritizedReplayBatch,  # noqa: F401
                     PrioritizedNStepReplayBatch)

__all__ = ["make_env", "MultiAgentEnv", "BatchMultiAgentEnv", "GraphedStep", "BaseScenario", "core", "scenarios", "MlpPolicy", "PolicyRollout",
           "PolicyTrajectory", "Actors", "PolicyLoop", "Critics", "TdTargets", "Values", "GaeResult", "gae", "gae_tensors",
           "adv_stats", "Minibatches", "OnPolicyBatch", "PpoLoss", "PpoLossResult", "ppo_loss_tensors",
           "Trainable", "MlpGradResult", "mlp_grad_tensors", "mlp_dinput_tensors", "DeviceAdam",
           "TdLoss", "TdLossResult", "td_loss_tensors", "ActorLoss", "RowsLayout", "PolicyRowsGradResult", "policy_rows_tensors",
           "policy_rows_grad_tensors", "PolyakTargets", "QLoss", "QLossResult", "QTargets", "q_loss_tensors",
           "ReplayBuffer", "ReplayBatch",
           "PrioritizedReplayBuffer", "PrioritizedReplayBatch", "NStepReplayBatch", "PrioritizedNStepReplayBatch"]
