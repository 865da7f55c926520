"""Policies in the loop for every env: `Actors` evaluates one MLP actor per agent for all B worlds in ONE launch of the standalone
MFMA actor kernel (mpe_actor_act, csrc/mpe_policy.hip) and hands back exactly the rows `env.step` takes; `PolicyLoop` drives
`act -> env.step` with device-side episode resets, eagerly or as one HIP graph.  DESIGN.md 2.10.

    pi = Actors(env, modules, mode="sample", seed=0)
    action = pi.act(obs_n, t)
    obs_n, rew_n, done_n, _ = env.step(action)
"""
import ctypes as C

import torch

from . import _abi
from .netset import _LW, Cache, NetSet, _actor_layers, check_tensor, pack_layers
from .rollout import _POLICY_MODES, _copy_struct, _step_many_env_check


def pack_actor16(module, n_out):
    """One actor in the packed layout of include/mpe_hip.h (MpeActorSet; netset.layout with a 16-wide last layer) -> a float32
    tensor on the module's device whose length is a multiple of 16."""
    return pack_layers(_actor_layers(module, n_out, "Actors")[0], _LW)


def joint_layout(obs_widths, movable, speaks, dim_c):
    """The columns of the centralised critic's joint row (include/mpe_hip.h, the joint-row rule; ReplayBatch.joint): every
    observation first, in agent order, then per agent its move row [5] if movable, directly followed by its utterance row [dim_c]
    if it speaks.  -> (off [A + 1], joint_width, col_move [A], col_utter [A]); a column an agent does not have is None."""
    off = [0]
    for d in obs_widths:
        off.append(off[-1] + int(d))
    col, col_move, col_utter = off[-1], [], []
    for m, sp in zip(movable, speaks):
        col_move.append(col if m else None)
        col += _abi.MPE_ACTION_DIM if m else 0
        col_utter.append(col if sp else None)
        col += dim_c if sp else 0
    return off, col, col_move, col_utter


def env_joint_layout(env, who):
    """joint_layout of an env's agents, read off the env as Actors and ReplayBuffer read it."""
    w = env.world
    off = getattr(env, "_obs_off", None)
    if off is None:
        raise _abi.MpeError("%s: this env has no device-side observation layout (env.fused is False)" % who)
    A = len(w.agents)
    speaks = [not a.silent for a in w.agents]
    return joint_layout([int(off[i + 1] - off[i]) for i in range(A)], [bool(a.movable) for a in w.agents], speaks,
                        int(w.dim_c) if any(speaks) else 0)


def _obs_blocks(net, obs_n, who, make, M=None):
    """-> (M, what make(A device pointers) built) for obs_n, a list of A contiguous float32 [M, D_i] blocks on the env's device (M:
    obs_n[0]'s rows, where the caller does not fix it); the blocks are checked, and make() is called, once per distinct set of
    blocks (net._ptrs)."""
    if len(obs_n) != net.A:
        raise _abi.MpeError("%s: %d observation blocks for %d agents" % (who, len(obs_n), net.A))
    if M is None:
        if not torch.is_tensor(obs_n[0]) or obs_n[0].dim() != 2:
            raise _abi.MpeError("%s: obs_n[0] is a contiguous float32 [M, %d] tensor on the env's device" % (who, net.obs_widths[0]))
        M = int(obs_n[0].shape[0])
    key = (M,) + tuple(o.data_ptr() if torch.is_tensor(o) else None for o in obs_n)

    def checked():
        for i, o in enumerate(obs_n):
            check_tensor(who, o, "obs_n[%d]" % i, [(M, net.obs_widths[i])], "the env's device", net.world.device)
        return make(key[1:])
    return M, net._ptrs.get(key, checked)


class _Rows(object):
    """The outputs of Actors.act_rows for one M."""
    __slots__ = ("moves", "utter", "logp", "ids", "logits", "joint", "action")


class Actors(NetSet):
    """Per-agent MLP actors for any env: `modules` is one nn.Sequential per agent, or one module every agent shares (Linear layers
    with ReLU / Tanh between them, at most 3 Linear layers, hidden widths <= 64, float32).  Agent i's first Linear takes its
    observation width D_i; its last gives 5 * movable + dim_c * speaks logits: a movable agent's first 5 are its move head, a
    speaking agent's last dim_c its utterance head, and each head gets `mode`'s rule (greedy / softmax / sample).
    logp / ids / logits = True: the same launch also fills pi.logp [A,B] (sum over the heads of log p[chosen]), pi.ids [2,A,B]
    int32 (move head, utterance head; -1 where an agent has no such head) and pi.logits [A,B,16] (raw last-layer outputs).
    The weights are packed again at every act() unless freeze() was called, so in-place optimiser updates are seen; agents
    handed the SAME module object share one packed copy.
    epsilon (mode="greedy" only): act() plays epsilon-greedy in the same launch (mpe_actor_act_explore, THE
    EXPLORATION RULE of include/mpe_hip.h: each head explores with probability E / 65536, E = round(epsilon * 65536), on the
    sample draws' own bits of (seed, world, t, agent)).  pi.epsilon is a plain attribute read at every act(), so a schedule is one
    assignment per step; 0 is mpe_actor_act itself.  act_rows never explores: a target is greedy.  Inside PolicyLoop.capture()
    the value is FROZEN at capture (a launch argument of the captured graph): re-capture to change it."""
    who, noun = "Actors", "actors"

    def __init__(self, env, modules, mode="sample", seed=0, logp=False, ids=False, logits=False, epsilon=0.0):
        if mode not in _POLICY_MODES:
            raise _abi.MpeError("Actors: mode is one of %s (got %r)" % (sorted(_POLICY_MODES), mode))
        self.mode, self.seed = mode, int(seed) & (2 ** 64 - 1)
        self.epsilon = epsilon
        self._epsilon("Actors")
        NetSet.__init__(self, env, modules)
        self.B = self.world.batch_size
        self._want = (bool(logp), bool(ids), bool(logits))
        self.moves = self.utter = self.logp = self.ids = self.logits = None
        self.off, self.joint_width, self.col_move, self.col_utter = joint_layout(self.obs_widths, self.movable, self.speaks, self.dim_c)
        self.rows = self.joint_rows = None
        self._rows, self._ptrs = Cache(), Cache(64)

    def _widths(self):
        w = self.world
        self.movable = [bool(a.movable) for a in w.agents]
        self.speaks = [not a.silent for a in w.agents]
        self.dim_c = int(w.dim_c) if any(self.speaks) else 0
        self.n_out = [_abi.MPE_ACTION_DIM * m + self.dim_c * s for m, s in zip(self.movable, self.speaks)]
        self.in_widths = self.obs_widths

    def _agent(self, i):
        if self.n_out[i] < 1:
            raise _abi.MpeError("Actors: agent %d neither moves nor speaks: it has no head" % i)
        if self.n_out[i] > _LW:
            raise _abi.MpeError("Actors: agent %d needs %d logits (5 * movable + dim_c * speaks), at most MPE_ACTOR_MAX_OUT = %d"
                                % (i, self.n_out[i], _LW))
        return "agent %d: movable = %s, speaks = %s, dim_c = %d" % (i, self.movable[i], self.speaks[i], self.dim_c)

    def _input_refusal(self, i, n, D):
        return "Actors: agent %d's actor takes %d inputs, its observation has %d" % (i, n, D)

    def _tail(self, aset):
        for i in range(self.A):
            aset.movable[i], aset.speaks[i] = int(self.movable[i]), int(self.speaks[i])
        aset.dim_c, aset.mode, aset.seed = self.dim_c, _POLICY_MODES[self.mode], self.seed

    def _new_rows(self, M):
        """the output tensors of one launch over M rows"""
        A, dev = self.A, self.world.device
        r = _Rows()
        r.moves = torch.zeros((A, M, _abi.MPE_ACTION_DIM), dtype=torch.float32, device=dev)
        r.utter = torch.zeros((A, M, self.dim_c), dtype=torch.float32, device=dev) if self.dim_c else None
        r.action = (r.moves, r.utter) if self.dim_c else r.moves
        logp, ids, logits = self._want
        r.logp = torch.zeros((A, M), dtype=torch.float32, device=dev) if logp else None
        r.ids = torch.zeros((2, A, M), dtype=torch.int32, device=dev) if ids else None
        r.logits = torch.zeros((A, M, _LW), dtype=torch.float32, device=dev) if logits else None
        r.joint = None
        return r

    def _buffers(self):
        if self.moves is None:
            r = self._new_rows(self.B)
            self.moves, self.utter, self.logp, self.ids, self.logits, self._action = r.moves, r.utter, r.logp, r.ids, r.logits, r.action

    def _ptr_array(self, ptrs):
        return (C.c_void_p * self.A)(*ptrs)

    def _epsilon(self, who):
        """self.epsilon, checked -> a float in [0, 1]"""
        try:
            eps = float(self.epsilon)
        except (TypeError, ValueError):
            eps = float("nan")
        if not 0.0 <= eps <= 1.0:      # (a NaN fails both)
            raise _abi.MpeError("%s: epsilon = %r (a number in [0, 1])" % (who, self.epsilon))
        if eps > 0.0 and self.mode != "greedy":
            raise _abi.MpeError("%s: epsilon = %r with mode %r (exploration replaces the choice of a mode=\"greedy\" set)"
                                % (who, self.epsilon, self.mode))
        return eps

    def act(self, obs_n, t=0, moves=None, logp=None):
        """One launch: every agent's rows for the observations obs_n (a list of [B, D_i] device tensors: env.step's / env.reset's
        own output qualifies) at global step t (the sample draws' key) -> the [A,B,5] move tensor, or (moves, utterances
        [A,B,dim_c]) where agents speak: what env.step takes, zero-copy.  The tensors are this object's own and are rewritten by
        the next act(); moves / logp: write those two into the caller's tensors instead (a trajectory's rows)."""
        self._buffers()
        wts, aset = self.packed()
        mv = self.moves if moves is None else moves
        lp = self.logp if logp is None else logp
        eps = self._epsilon("Actors.act")
        arr = _obs_blocks(self, obs_n, "Actors.act", self._ptr_array, self.B)[1]
        out = (mv.data_ptr(), self.utter.data_ptr() if self.utter is not None else None,
               self.ids.data_ptr() if self.ids is not None else None, lp.data_ptr() if lp is not None else None,
               self.logits.data_ptr() if self.logits is not None else None, _abi.raw_stream(self.world.device))
        if eps > 0.0:
            _abi.check(_abi.lib().mpe_actor_act_explore(C.byref(aset), arr, self.B, int(t), int(self.world.world_offset), eps, *out),
                       "mpe_actor_act_explore")
        else:
            _abi.check(_abi.lib().mpe_actor_act(C.byref(aset), arr, self.B, int(t), int(self.world.world_offset), *out), "mpe_actor_act")
        del wts      # (stream-ordered: the caching allocator reuses the block only behind the launch)
        if moves is None:
            return self._action
        return (mv, self.utter) if self.dim_c else mv

    def _rows_out(self, M, joint):
        """act_rows' own output tensors, one set per M (the [B]-sized buffers of act() are not touched)."""
        r = self._rows.get(M, lambda: self._new_rows(M))
        if joint and r.joint is None:
            r.joint = torch.zeros((M, self.joint_width), dtype=torch.float32, device=self.world.device)
        return r

    def act_rows(self, obs_n, t=0, row_offset=0, joint=None, _packed=None):
        """act() over M rows of any origin (M = obs_n[0].shape[0]: a sampled minibatch's next_obs_n) in one launch
        (mpe_actor_act_rows): row m's SAMPLE draws are those of world row_offset + m at step t.  joint=True: the same launch also
        writes the centralised critic's input rows [M, joint_width] -- every observation, then the action rows just decided, in
        ReplayBatch.joint's columns (self.off, col_move, col_utter) -- into a tensor of this object's; joint=a contiguous float32
        [M, >= joint_width] device tensor: into that one.  -> what act() returns, [A,M,...]; self.joint_rows is the joint tensor
        (None without joint) and self.rows holds every output of the call (moves, utter, logp, ids, logits, joint).  The tensors
        are cached per M and rewritten by the next act_rows of that M.  (_packed: the pair to read in place of packed().)"""
        M, arr = _obs_blocks(self, obs_n, "Actors.act_rows", self._ptr_array)
        dev = self.world.device
        own = joint is True
        if joint is not None and joint is not False and not own:
            if not torch.is_tensor(joint) or joint.dtype != torch.float32 or joint.dim() != 2 or joint.shape[0] != M or \
                    joint.shape[1] < self.joint_width or not joint.is_contiguous() or joint.device != dev:
                raise _abi.MpeError("Actors.act_rows: joint is True or a contiguous float32 [%d, >= %d] tensor on the env's device"
                                    % (M, self.joint_width))
        r = self._rows_out(M, own)
        jt = r.joint if own else joint if torch.is_tensor(joint) else None
        wts, aset = _packed if _packed is not None else self.packed()
        _abi.check(_abi.lib().mpe_actor_act_rows(
            C.byref(aset), arr, M, int(t), int(row_offset), r.moves.data_ptr(), r.utter.data_ptr() if r.utter is not None else None,
            r.ids.data_ptr() if r.ids is not None else None, r.logp.data_ptr() if r.logp is not None else None,
            r.logits.data_ptr() if r.logits is not None else None, jt.data_ptr() if jt is not None else None,
            int(jt.shape[1]) if jt is not None else 0, _abi.raw_stream(dev)), "mpe_actor_act_rows")
        del wts
        self.rows, self.joint_rows = r, jt
        return r.action

    def train_forward(self, obs_n, packed):
        """The forward Trainable runs, on the packed pair it hands to the backward: act_rows -> (M, per agent the live columns
        [M, n_out_i] of the launch's logits, the input rows)."""
        self.act_rows(obs_n, _packed=packed)
        z = self.rows.logits
        return int(obs_n[0].shape[0]), [z[i, :, :n].clone(memory_format=torch.contiguous_format) for i, n in enumerate(self.n_out)], list(obs_n)

    def reference(self, obs_n):
        """The fp64 torch forward pass, on whatever device the modules and obs_n are: per agent (move logits [B,5] or None,
        utterance logits [B,dim_c] or None)."""
        import copy
        out = []
        for i, o in enumerate(obs_n):
            m = copy.deepcopy(self.modules[i]).double()
            with torch.no_grad():
                z = m(torch.as_tensor(o).to(next(m.parameters()).device).double())
            out.append((z[:, :_abi.MPE_ACTION_DIM] if self.movable[i] else None,
                        z[:, z.shape[1] - self.dim_c:] if self.speaks[i] else None))
        return out


class LoopTrajectory(object):
    """What PolicyLoop.run recorded: obs[t][i] [B, D_i], rew [T,A,B], done [T,A,B] (the outputs of step t), act [T,A,B,5] (the rows
    applied at step t), utter [T,A,B,dim_c] or None, logp [T,A,B] or None.  Recorded with run(T, values=V) only: obs_in[t][i]
    [B, D_i] (the observation step t was decided on), val [T,A,B], boot [K,A,B], episode_len, episode_phase (onpolicy.py)."""

    def __init__(self, env, pi, T):
        w, off = env.world, env._obs_off
        A, B, dev = pi.A, pi.B, w.device
        self.T = T
        self.obs_flat = torch.zeros((T, int(off[-1]) * B), dtype=torch.float32, device=dev)
        self.obs = [[self.obs_flat[t, off[i] * B: off[i + 1] * B].view(B, off[i + 1] - off[i]) for i in range(A)] for t in range(T)]
        self.rew = torch.zeros((T, A, B), dtype=torch.float32, device=dev)
        self.done = torch.zeros((T, A, B), dtype=torch.bool, device=dev)
        self.act = torch.zeros((T, A, B, _abi.MPE_ACTION_DIM), dtype=torch.float32, device=dev)
        self.utter = torch.zeros((T, A, B, pi.dim_c), dtype=torch.float32, device=dev) if pi.dim_c else None
        self.logp = torch.zeros((T, A, B), dtype=torch.float32, device=dev) if pi._want[0] else None


class PolicyLoop(object):
    """The closed loop `act_n = policy(obs_n); env.step(act_n)` on the device: per step one actor launch (Actors.act) and one
    env.step, and every episode_len global steps, first, the device-side reset RandomRollout.enqueue makes (mpe_reset /
    mpe_reset_rows with `seed`'s draws, the comm state zeroed) and the observation of the reset state.  Works wherever env.step
    is a device step: the built-in scenarios at any size, row-program envs, traced reference-style files; refuses what
    step_many refuses, by the same names.  run() calls continue one step count and episode clock."""

    def __init__(self, env, actors, episode_len=25, seed=None):
        if not isinstance(actors, Actors):
            raise _abi.MpeError("PolicyLoop: actors is an Actors(env, modules, ...)")
        if actors.env is not env:
            raise _abi.MpeError("PolicyLoop: the Actors were built for another env")
        _step_many_env_check(env)
        if int(episode_len) and not env._device_restart_ok:
            raise _abi.MpeError("PolicyLoop(episode_len > 0): the resets are world.reset_uniform's device draws; this env's "
                                "reset_world is not that -- use episode_len = 0 and reset it yourself")
        env._ensure_buffers()
        self.env, self.world, self.pi = env, env.world, actors
        self.episode_len = int(episode_len)
        self.seed = int(env.world.seed if seed is None else seed) & (2 ** 64 - 1)
        self._prog = getattr(env, "_prog", None)
        self._lr = float(getattr(env._scenario, "landmark_range", 1.0))
        self._gen_desc = _copy_struct(self.world.scenario_desc(_abi.MPE_SCN_GENERIC))
        self.t = 0
        self.obs_n = None      # the observation the next decision is taken on (None: observed at the next step)

    def device_reset(self, episode):
        """Restart every world with the draws of (seed, episode) on the device and observe the new state -> obs_n."""
        env, w, L = self.env, self.world, _abi.lib()
        st = _abi.raw_stream(w.device)
        b = env._sets[0].bufs
        if self._prog is not None:
            _abi.check(L.mpe_reset_rows(C.byref(self._gen_desc), C.byref(b), self._prog.ref, w.batch_size, None, self._lr, self.seed,
                                        int(episode), int(w.world_offset), st), "mpe_reset_rows")
        else:
            _abi.check(L.mpe_reset(C.byref(self._gen_desc), C.byref(b), w.batch_size, None, self._lr, self.seed, int(episode),
                                   int(w.world_offset), st), "mpe_reset")
        if env._comm is not None:
            env._comm.zero_()
        return self._observe()

    def _observe(self):
        env = self.env
        out = env._next_set()
        env._observe_into(out)
        return list(out.obs_n)

    def _mark_stale(self):
        env = self.env
        if self.episode_len:      # (device-side resets bypass Scenario.reset_world: re-derived before the next Python-API step)
            env._scenario_state_stale = True
            if env.episode_step is not None:
                env.episode_step.fill_(self.t % self.episode_len)

    def _replay_check(self, replay):
        from .replay import ReplayBuffer
        if not isinstance(replay, ReplayBuffer) or replay.env is not self.env:
            raise _abi.MpeError("PolicyLoop: replay is a ReplayBuffer(env, steps) built for this loop's env")

    def step(self, traj=None, k=0, replay=None, values=None):
        """One step of the loop at global step self.t -> env.step's outputs.  replay: a ReplayBuffer that takes the step's
        transition (the observation decided on, the action applied, env.step's outputs) with one more launch.  values: run()'s
        record of a Values along traj (onpolicy._ValueRecord)."""
        env, pi = self.env, self.pi
        if self.episode_len and self.t % self.episode_len == 0:
            self.obs_n = self.device_reset(self.t // self.episode_len)
        elif self.obs_n is None:
            self.obs_n = self._observe()
        if values is not None:
            values.decided(k)
        if traj is not None:
            action = pi.act(self.obs_n, self.t, moves=traj.act[k], logp=traj.logp[k] if traj.logp is not None else None)
        else:
            action = pi.act(self.obs_n, self.t)
        out = env.step(action)
        if replay is not None:
            # the env double-buffers its output sets, so the step wrote beside the observation it was decided on
            if any(a.data_ptr() == b.data_ptr() for a, b in zip(self.obs_n, out[0])):
                raise _abi.MpeError("PolicyLoop: env.step overwrote the observation the action was chosen on; nothing was pushed")
            replay.push(self.obs_n, action, out[0], out[1], out[2])
        self.obs_n = out[0]
        if traj is not None:
            o = env._sets[env._flip]
            traj.obs_flat[k].copy_(o.obs)
            traj.rew[k].copy_(o.rew)
            traj.done[k].copy_(o.done)
            if traj.utter is not None:
                traj.utter[k].copy_(pi.utter)
        self.t += 1
        if values is not None:
            values.stepped(k, out[0])
        return out

    def run(self, T, record=True, replay=None, values=None):
        """T steps.  record: -> a LoopTrajectory (three device copies per step); False: -> the last step's env.step outputs.
        replay: every step's transition is pushed to that ReplayBuffer (one launch per step).  values: an onpolicy.Values of this
        env; the trajectory additionally holds obs_in[t][i] (the observation step t was decided on), val [T,A,B] (V of it), boot
        [K,A,B] (V of the output observation of each of the K segment-ending steps), episode_len and episode_phase: what
        onpolicy.gae takes.  T + K more launches and one more copy per step."""
        _step_many_env_check(self.env)
        if replay is not None:
            self._replay_check(replay)
        if values is not None and not record:
            raise _abi.MpeError("PolicyLoop.run: values= records V along the trajectory; it needs record=True")
        traj = LoopTrajectory(self.env, self.pi, int(T)) if record else None
        if values is not None:
            from .onpolicy import _ValueRecord
            values = _ValueRecord(self, traj, values)
        out = None
        for k in range(int(T)):
            out = self.step(traj, k, replay, values)
        self._mark_stale()
        return traj if record else out

    def capture(self, T, replay=None):
        """The next T steps (from self.t, the current state) as ONE HIP graph: a straight line of kernels -- reset, observe, act,
        step -- with nothing recorded.  -> an object whose replay() runs them and advances this loop's step count by T; the
        draw keys and episode numbers are those of the captured steps (a replay repeats them: capture a multiple of episode_len
        steps from an episode start for a periodic rollout, as RandomRollout.capture).  The weights are frozen for the capture
        (freeze() again and re-capture after a torch update of the modules); with a DeviceAdam (optim.py) the actors already read
        the optimiser's live buffer, the captured launches read it too, and the graph needs NO re-capture after an update.  Two warm-up steps really run in front of the capture; the state and the
        step count are put back.  replay: every captured step pushes its transition to that ReplayBuffer; the
        push reads and advances the buffer's device-side step count, so each replay() fills the next T slots (the warm-up steps'
        pushes are taken back through the buffer's _mark / _rewind hooks: the count is restored -- and a prioritized buffer's
        priorities, tree and pmax --, the two slots they wrote are the first two the graph writes)."""
        _step_many_env_check(self.env)
        env, w, pi = self.env, self.world, self.pi
        if replay is not None:
            self._replay_check(replay)
            replay._alloc()
        if pi.attached() is None:
            pi.freeze()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream(device=w.device)
        s.wait_stream(torch.cuda.current_stream(w.device))
        t0, obs0, flip0 = self.t, self.obs_n, env._flip
        with torch.cuda.stream(s):
            if self.obs_n is None and not (self.episode_len and self.t % self.episode_len == 0):
                self.obs_n = obs0 = self._observe()
                flip0 = env._flip
            pos, vel = w.pos.clone(), w._vel_all.clone()
            comm = env._comm.clone() if env._comm is not None else None
            keep = [o.clone() for o in obs0] if obs0 is not None else None
            choice = w.choice_i32.clone() if w.choice_i32 is not None else None
            mark, count = (replay._mark(2), replay.count) if replay is not None else (None, 0)
            for _ in range(2):      # code objects and allocations outside the capture
                self.step(replay=replay)
            if replay is not None:
                replay.count = count
                replay._rewind(mark)
            w.pos.copy_(pos)
            w._vel_all.copy_(vel)
            if comm is not None:
                env._comm.copy_(comm)
            if choice is not None:
                w.choice_i32.copy_(choice)
            if keep is not None:
                for dst, src in zip(obs0, keep):
                    dst.copy_(src)
            self.t, self.obs_n, env._flip = t0, obs0, flip0
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=s):
                for _ in range(int(T)):
                    self.step(replay=replay)
        torch.cuda.current_stream(w.device).wait_stream(s)
        self.t = t0
        if replay is not None:
            replay.count = count      # (captured launches have not run: replay() counts them)
        return _LoopGraph(g, self, int(T), self.obs_n, env._flip, replay)


class _LoopGraph(object):
    def __init__(self, graph, loop, T, obs_n, flip, replay=None):
        self.graph, self.loop, self.T, self._obs_n, self._flip, self._replay = graph, loop, T, obs_n, flip, replay

    def replay(self):
        loop = self.loop
        self.graph.replay()
        loop.t += self.T
        if self._replay is not None:
            self._replay.count += self.T
        loop.obs_n, loop.env._flip = self._obs_n, self._flip
        loop._mark_stale()
        for out in loop.env._sets:
            out.act_ptr = None
