"""The task layer of a closed learning loop on the GPU: ``WalkingTask`` decides, per world and control tick, what the tick was
worth, whether the episode ended and why, and writes the observation row (``csrc/nmf_task.hip``; specification
``tests/task_spec.py``); ``TaskEnv`` is the loop around it — drive, step, update, reset what ended — without a host
synchronisation, as one captured graph per tick on request.

Build-defined and pinned by nothing (the reference ships no tasks; flygym 1.x's Gymnasium environments are its form, and nothing is
claimed about matching them).  The statement of the rule is include/nmf.h (``nmf_task_update``).
"""

from __future__ import annotations

import ctypes

import numpy as np

from . import _native
from ._handle import NativeHandle, _field_view, check_params, fly_batch, leg_segments, reset_mask
from .anatomy import LEGS

__all__ = ["WalkingTask", "TaskEnv", "REASONS"]

# the bits of ``reason`` / ``last_reason`` (NMF_TASK_ of include/nmf.h); 0 in ``last_reason`` is the time limit
REASONS = dict(nonfinite=1, tilted=2, airborne=4, height=8, out_of_arena=16, goal=32)
POWER_BITS = 10
MAX_ACT, MAX_Q = 64, 256


class _TaskParams(ctypes.Structure):
    """``nmf_task_params`` of include/nmf.h."""

    _fields_ = [("root_seg", ctypes.c_int32), ("n_act", ctypes.c_int32), ("n_q", ctypes.c_int32), ("tilt_ticks", ctypes.c_int32),
                ("airborne_ticks", ctypes.c_int32), ("max_ticks", ctypes.c_int32), ("grace_ticks", ctypes.c_int32),
                ("cos_max_tilt", ctypes.c_float), ("z_min", ctypes.c_float), ("z_max", ctypes.c_float), ("arena", ctypes.c_float * 4),
                ("goal_radius2", ctypes.c_float), ("power_clip", ctypes.c_float), ("thr2", ctypes.c_float * 6), ("alive", ctypes.c_float),
                ("w_progress", ctypes.c_float), ("w_power", ctypes.c_float), ("w_tilt", ctypes.c_float), ("bonus_goal", ctypes.c_float),
                ("penalty_fail", ctypes.c_float)]


class WalkingTask(NativeHandle):
    """The walking task of one fly of a :class:`~flygym_amd.HIPSimulation` on the GPU (``nmf_task_*``): reward, termination,
    truncation, episode accounts and the observation row, one kernel launch per control tick.

    Build-defined and pinned by nothing; the rule is stated step by step in include/nmf.h (``nmf_task_update``) and specified in
    numpy in tests/task_spec.py, which the kernel equals bit for bit.  One :meth:`update` reads the batch as it stands (the root
    segment's pose, ``qvel[0:6]``, the chosen actuators' forces and joint velocities, the legs' contact sensors, the chosen joint
    angles) and :attr:`course` and :attr:`goal`, and per world, in float32::

        bad      = a value read is NaN or +-Inf            -> reason nonfinite alone, reward -penalty_fail, a row of zeros
        progress = (position - position at the last update) . course                  (0 on the first update of an episode)
        up_z     = 1 - 2 (qx^2 + qy^2);  tilt_count grows while up_z < cos(max_tilt), else 0
        airborne_count grows while no leg touches with a force above contact_force_thr, else 0
        power    = sum_a clip(|force_a * qvel_a|, 0, power_clip), summed as integers in units of 2^-10
        reason   = tilted (tilt_count >= tilt_ticks) | airborne (airborne_count >= airborne_ticks) | height (z outside z_range)
                   | out_of_arena | goal (within goal_radius of goal);  the first three not in the first grace_ticks updates
        terminated = reason != 0;  truncated = not terminated and the episode is max_ticks long;  done = either
        reward   = alive + w_progress progress - w_power power - w_tilt (1 - up_z) + bonus_goal [goal] - penalty_fail [another reason]
        obs      = gravity direction, linear and angular velocity, goal direction (x, y) — all in the body frame — and height
                   (12 floats), the six contact flags, (angle - obs_mean) / obs_std per observed dof

    A world that is done starts its next episode by itself: the accounts are latched into ``last_return``, ``last_length`` and
    ``last_reason`` (0: the time limit), ``episodes`` (and ``successes`` for a goal) count up, the accumulators return to their
    start values and ``fresh`` is set.  The physics is not touched: pass :attr:`done` to ``sim.reset_worlds`` and to the
    controllers' ``reset`` — it is the mask they take, on the device (what :class:`TaskEnv` does).

    Args:
        sim: the batch; for a world with several flies ``sim.for_fly(fly_name)``.
        fly_name: the fly that walks.
        actuators: joint dofs (``JointDOF`` or names) whose position actuators enter the power sum (1..64); default the fly's
            position actuators on leg dofs.
        obs_dofs: joint dofs observed (1..256); default as ``HeadStabilizer.input_dofs``: the leg dofs that have position actuators.
        obs_mean, obs_std: per observed dof (default 0 and 1).
        contact_force_thr: per leg pair front / middle / hind, in the contact sensors' force unit (``HeadStabilizer``'s).
        max_tilt: degrees between the body's z axis and the vertical beyond which a tick counts as tilted.
        tilt_ticks, airborne_ticks, grace_ticks, max_ticks: in updates.
        z_range: ``(z_min, z_max)`` of the root segment; arena: ``(x_min, x_max, y_min, y_max)``.
        goal_radius: 0 switches the goal off.
        power_clip: per actuator, in force unit times rad/s.
        alive, w_progress, w_power, w_tilt, bonus_goal, penalty_fail: the reward's weights.

    The defaults of ``max_tilt``, ``tilt_ticks``, ``airborne_ticks``, ``grace_ticks``, ``z_range`` and ``power_clip`` lie outside
    what 256 flies walking under ``TurningCPG`` on flat ground and on the blocks terrain were measured to do, by the margins
    profiles/task_summary.md states.

    ``reward``, ``ep_return``, ``last_return`` ``(n,)``, ``obs`` ``(n, 12 + 6 + n_q)``, ``prev_xy``, ``course``, ``goal`` ``(n, 2)``
    float32, ``terminated``, ``truncated``, ``done``, ``fresh`` ``(n,)`` uint8 and ``reason``, ``ep_length``, ``last_length``,
    ``last_reason``, ``tilt_count``, ``airborne_count``, ``episodes``, ``successes`` ``(n,)`` int32 are zero-copy views of the device
    state: every update rewrites them (clone to keep a value), and they are writable between launches.  Every method but
    :meth:`stats` is stream-ordered device work on the simulation's stream; :meth:`update` is one launch and can be captured in a
    graph.  Close the task before its simulation.
    """

    _destroy_entry, _noun = "nmf_task_destroy", "task"
    _FLOATS = ("reward", "obs", "ep_return", "last_return", "prev_xy", "course", "goal")
    _BYTES = ("terminated", "truncated", "done", "fresh")
    _INTS = ("reason", "ep_length", "last_length", "last_reason", "tilt_count", "airborne_count", "episodes", "successes")
    _views = _FLOATS + _BYTES + _INTS
    OBS_BODY = 12

    def __init__(self, sim, fly_name: str, *, actuators=None, obs_dofs=None, obs_mean=None, obs_std=None,
                 contact_force_thr=(0.5, 1.0, 3.0), max_tilt: float = 60.0, tilt_ticks: int = 5, airborne_ticks: int = 5,
                 grace_ticks: int = 15, max_ticks: int = 500, z_range=(0.75, 2.0), arena=(-1e3, 1e3, -1e3, 1e3), goal_radius: float = 0.0,
                 power_clip: float = 2048.0, alive: float = 0.0, w_progress: float = 1.0, w_power: float = 0.0, w_tilt: float = 0.0,
                 bonus_goal: float = 0.0, penalty_fail: float = 0.0):
        sim = fly_batch(sim, fly_name, resolve=False)
        if fly_name not in sim.world.fly_lookup:
            raise ValueError(f"no fly named {fly_name!r} in this simulation ({', '.join(sim.world.fly_lookup)})")
        fly = sim.world.fly_lookup[fly_name]
        self.sim, self.fly_name, self.n_worlds = sim, fly_name, int(sim.n_worlds)
        all_dofs = [d.name for d in fly.get_jointdofs_order()]
        name_of = lambda d: d if isinstance(d, str) else d.name
        leg_dofs = [d for d in fly.get_actuated_jointdofs_order("position") if d.child.pos in LEGS]
        self.actuators = [name_of(d) for d in (leg_dofs if actuators is None else actuators)]
        self.obs_dofs = [name_of(d) for d in (leg_dofs if obs_dofs is None else obs_dofs)]
        ids = {a["jointdof"].name: i for i, a in enumerate(fly.actuators) if a["kind"] == "position"}
        for d in self.actuators:
            if d not in ids:
                raise ValueError(f"{d} has no position actuator on this fly")
        missing = [d for d in self.obs_dofs if d not in all_dofs]
        if missing:
            raise ValueError(f"the fly has no joint dof {missing[0]!r}")
        if not 1 <= len(self.actuators) <= MAX_ACT:
            raise ValueError(f"actuators takes 1..{MAX_ACT} joint dofs, got {len(self.actuators)}")
        if not 1 <= len(self.obs_dofs) <= MAX_Q:
            raise ValueError(f"obs_dofs takes 1..{MAX_Q} joint dofs, got {len(self.obs_dofs)}")
        self._act = np.array([ids[d] for d in self.actuators], dtype=np.int32)
        self._act_dof = np.array([all_dofs.index(d) for d in self.actuators], dtype=np.int32)
        self._obs_dof = np.array([all_dofs.index(d) for d in self.obs_dofs], dtype=np.int32)
        n_q = len(self.obs_dofs)
        self.n_act, self.n_q, self.obs_width = len(self.actuators), n_q, self.OBS_BODY + 6 + n_q
        self._mean = np.zeros(n_q, dtype=np.float32) if obs_mean is None else np.ascontiguousarray(obs_mean, dtype=np.float32)
        std = np.ones(n_q, dtype=np.float32) if obs_std is None else np.ascontiguousarray(obs_std, dtype=np.float32)
        if self._mean.shape != (n_q,) or std.shape != (n_q,):
            raise ValueError(f"obs_mean and obs_std take one value per observed dof ({n_q}), got {self._mean.shape} and {std.shape}")
        if not (std > 0).all():
            raise ValueError("obs_std must be positive")
        self._inv_std = (1.0 / std.astype(np.float64)).astype(np.float32)       # divided in float64, rounded once
        if len(contact_force_thr) != 3:
            raise ValueError(f"contact_force_thr takes three values (front, middle, hind legs), got {contact_force_thr!r}")
        if len(z_range) != 2:
            raise ValueError(f"z_range takes (z_min, z_max), got {z_range!r}")
        if len(arena) != 4:
            raise ValueError(f"arena takes (x_min, x_max, y_min, y_max), got {arena!r}")
        if not 0.0 <= float(max_tilt) <= 180.0:
            raise ValueError(f"max_tilt must be in 0..180 degrees, got {max_tilt!r}")
        if not float(goal_radius) >= 0.0:
            raise ValueError(f"goal_radius must not be negative, got {goal_radius!r}")
        thr = [float(contact_force_thr["fmh".index(leg[1])]) for leg in LEGS]
        self.thr2 = np.array([t * t for t in thr], dtype=np.float32)
        self.root_seg, _ = leg_segments(fly, LEGS)
        check_params(_TaskParams, "nmf_task_params_size", "tasks.py")
        self._params = _TaskParams(
            self.root_seg, self.n_act, n_q, int(tilt_ticks), int(airborne_ticks), int(max_ticks), int(grace_ticks),
            float(np.float32(np.cos(np.deg2rad(float(max_tilt))))), float(z_range[0]), float(z_range[1]),
            (ctypes.c_float * 4)(*(float(v) for v in arena)), float(np.float32(float(goal_radius) ** 2)), float(power_clip),
            (ctypes.c_float * 6)(*self.thr2.tolist()), float(alive), float(w_progress), float(w_power), float(w_tilt), float(bonus_goal),
            float(penalty_fail))
        h = self._create("nmf_task_create", sim._batch_h, ctypes.byref(self._params), self._act.ctypes.data, self._act_dof.ctypes.data,
                         self._obs_dof.ctypes.data, self._mean.ctypes.data, self._inv_std.ctypes.data)
        n = self.n_worlds
        for which, name in enumerate(self._views):
            typestr = "<f4" if name in self._FLOATS else "|u1" if name in self._BYTES else "<i4"
            view = _field_view(sim, _native.lib().nmf_task_field_ptr, h, which, typestr)
            setattr(self, name, view if view.shape[1] > 1 else view.reshape(n))

    def update(self):
        """One update of every world from the batch as it stands.  One kernel launch, no allocation — capturable.  Returns the
        views ``(obs, reward, terminated, truncated)``."""
        _native.check(_native.lib().nmf_task_update(self._handle(), self.sim._stream()))
        return self.obs, self.reward, self.terminated, self.truncated

    def reset(self, mask=None) -> None:
        """The worlds of ``mask`` (``(n_worlds,)`` bool, numpy or torch; default all) get a new episode and empty statistics: every
        view zeroed except :attr:`course` and :attr:`goal`, ``fresh`` set; the others keep their state."""
        h = self._handle()
        m = reset_mask(mask, self.n_worlds, self.sim)
        _native.check(_native.lib().nmf_task_reset(h, None if m is None else m.data_ptr(), self.sim._stream()))

    def _rows(self, name, x):
        """``x`` — one shared row ``(2,)`` / ``(1, 2)`` or one per world ``(n_worlds, 2)``, numpy, torch or a sequence — as a float32
        tensor on the simulation's device that broadcasts over the worlds."""
        t = self.sim._torch
        if not isinstance(x, t.Tensor):
            x = t.as_tensor(np.array(x, dtype=np.float32))
        if tuple(x.shape) not in ((self.n_worlds, 2), (1, 2), (2,)):
            raise ValueError(f"{name} must have shape ({self.n_worlds}, 2), (1, 2) or (2,), got {tuple(x.shape)}")
        return x.to(device=self.sim.device, dtype=t.float32).reshape(-1, 2)

    def set_course(self, course, normalise: bool = True) -> None:
        """The direction progress is measured along: one shared row or one per world, normalised here (in torch, on the device)
        unless ``normalise`` is False — then the rows are copied as they are.  A zero row earns no progress."""
        self._handle()
        rows = self._rows("course", course)
        if normalise:
            rows = rows / (rows * rows).sum(dim=1, keepdim=True).sqrt().clamp_min(1e-30)
        self.course.copy_(rows)

    def set_goal(self, goal) -> None:
        """The goal point: one shared row or one per world, copied into :attr:`goal`."""
        self._handle()
        self.goal.copy_(self._rows("goal", goal))

    def stats(self) -> dict:
        """The one method that synchronises with the host: ``episodes`` and ``successes`` (sums over the worlds), ``mean_return``
        and ``mean_length`` over the last finished episode of every world that finished one, and ``reasons``: how many of those
        ended for each reason (``time_limit`` for none; an episode can carry several bits)."""
        self._handle()
        episodes, successes = self.episodes.cpu().numpy(), self.successes.cpu().numpy()
        finished = episodes > 0
        last = self.last_reason.cpu().numpy()[finished]
        reasons = {name: int(((last & bit) != 0).sum()) for name, bit in REASONS.items()}
        reasons["time_limit"] = int((last == 0).sum())
        mean = lambda a: float(a.cpu().numpy()[finished].mean()) if finished.any() else float("nan")
        return dict(episodes=int(episodes.sum()), successes=int(successes.sum()), mean_return=mean(self.last_return),
                    mean_length=mean(self.last_length), reasons=reasons)


class TaskEnv:
    """The loop around a :class:`WalkingTask`: one :meth:`step` is one control tick of every world, with no host synchronisation
    anywhere::

        controller.drive <- action                       (if given)
        controller.step(steps_per_tick)                  the controller's table and the physics
        task.update()                                    reward, termination, the observation row
        sim.reset_worlds(task.done); controller.reset(task.done); h.reset(task.done) for h in also_reset

    Args:
        sim: the batch the controller steps.
        controller: anything with ``.drive`` ``(n, 2)``, ``.step(n)`` and ``.reset(mask)``: ``TurningCPG``, ``HybridTurningCPG``,
            ``RuleBasedController``.
        task: the :class:`WalkingTask` of the same batch.
        steps_per_tick: physics steps per control tick.
        also_reset: further handles whose ``reset(mask)`` follows the task's ``done`` (plume, navigator, odometry, motion detectors).
        capture: capture the tick once — after one eager warm-up tick, which counts as a tick of the episodes — into a
            ``torch.cuda.CUDAGraph``, on one stream as one linear chain; :meth:`step` then copies the action into a static buffer
            and replays.

    Aliasing: ``step`` returns the task's own views ``(obs, reward, terminated, truncated, info)``, ``info`` a dict of the views
    ``reason``, ``episodes``, ``last_return`` and ``last_length``.  Every tick rewrites them: clone what has to outlive the next
    ``step``.

    The reset convention: for a world that ended, the row returned by that ``step`` is its terminal observation (``terminated`` or
    ``truncated`` is set, ``task.fresh`` too), and its physics and controller are already back at the keyframe; the row of the
    next ``step`` is the first of its new episode.  A fly reset to the keyframe is dropped from its spawn height: the task's
    ``grace_ticks`` cover the landing.
    """

    def __init__(self, sim, controller, task, steps_per_tick: int = 20, also_reset=(), capture: bool = False):
        for name in ("drive", "step", "reset"):
            if not hasattr(controller, name):
                raise TypeError(f"the controller needs .drive, .step(n) and .reset(mask): {type(controller).__name__} has no .{name}")
        if not isinstance(task, WalkingTask):
            raise TypeError(f"task must be a WalkingTask, got {type(task).__name__}")
        if task.sim is not sim:
            raise ValueError("the task belongs to another batch than sim")
        if getattr(controller, "sim", sim) is not sim:
            raise ValueError("the controller belongs to another batch than sim")
        if int(steps_per_tick) < 1:
            raise ValueError(f"steps_per_tick must be at least 1, got {steps_per_tick}")
        for h in also_reset:
            if not hasattr(h, "reset"):
                raise TypeError(f"also_reset takes handles with .reset(mask): {type(h).__name__} has none")
        self.sim, self.controller, self.task = sim, controller, task
        self.steps_per_tick, self.also_reset, self.capture = int(steps_per_tick), tuple(also_reset), bool(capture)
        self.info = dict(reason=task.reason, episodes=task.episodes, last_return=task.last_return, last_length=task.last_length)
        t = sim._torch
        self._action = t.ones((task.n_worlds, 2), dtype=t.float32, device=sim.device)      # the captured tick's static input
        self._graph = None

    def _tick(self) -> None:
        self.controller.step(self.steps_per_tick)
        self.task.update()
        done = self.task.done
        self.sim.reset_worlds(done)
        self.controller.reset(done)
        for h in self.also_reset:
            h.reset(done)

    def _checked(self, action):
        t = self.sim._torch
        shape = (self.task.n_worlds, 2)
        if not isinstance(action, t.Tensor) or tuple(action.shape) != shape or action.dtype != t.float32 or action.device != t.device(self.sim.device):
            got = f"{tuple(action.shape)} {action.dtype} on {action.device}" if isinstance(action, t.Tensor) else type(action).__name__
            raise ValueError(f"action must be a float32 tensor of shape {shape} on {self.sim.device}, got {got}")
        return action

    def step(self, action=None):
        """One control tick; ``action`` ``(n_worlds, 2)`` float32 on the simulation's device is copied into ``controller.drive``
        (None: the drive stays).  Returns ``(obs, reward, terminated, truncated, info)``: views, see the class."""
        task = self.task
        task._handle()
        if action is not None:
            self._checked(action)
        if not self.capture:
            if action is not None:
                self.controller.drive.copy_(action)
            self._tick()
        else:
            self._action.copy_(self.controller.drive if action is None else action)
            if self._graph is None:
                t = self.sim._torch
                self.controller.drive.copy_(self._action)
                self._tick()                                   # the warm-up tick: every kernel of the chain has run before the capture
                graph = t.cuda.CUDAGraph()
                with t.cuda.graph(graph):
                    self.controller.drive.copy_(self._action)
                    self._tick()
                self._graph = graph
            else:
                self._graph.replay()
        return task.obs, task.reward, task.terminated, task.truncated, self.info

    def reset(self):
        """Everything starts again — the physics, the controller, the task and the handles of ``also_reset`` — and the first
        observation is returned: one :meth:`WalkingTask.update` of the keyframe pose, which counts as the first tick of the
        episodes."""
        self.sim.reset()
        self.controller.reset()
        self.task.reset()
        for h in self.also_reset:
            h.reset()
        self.task.update()
        return self.task.obs
