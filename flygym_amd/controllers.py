"""Controllers that produce position-actuator targets for the batched engine: the open-loop ``TripodCPG`` table builder, the
closed-loop, steerable ``TurningCPG`` whose state lives on the GPU, and ``HybridTurningCPG``, which adds flygym 1.x's two sensory
rules (retraction, stumbling) to it (both at the end of this docstring).

``TripodCPG`` is the "position-actuated CPG tripod gait" of BASELINE config 2.  The reference snapshot has
no CPG (flygym 2.0.1 dropped flygym 1.x's controllers), so this one is build-defined:

* six phase oscillators, one per leg, advancing at ``frequency`` (default 12 Hz); tripod phase biases
  ``{lf, rm, lh} = 0`` and ``{rf, lm, rh} = pi``;
* each leg's seven actuated joint angles are a periodic function of its phase: one step cycle cut from the
  Spotlight walking clip (the mean stride between the clip's swing onsets of that leg), resampled on a uniform
  phase grid and blended to be periodic;
* world ``w`` of ``n_worlds`` starts with the global phase offset ``2 pi w / n_worlds`` — deterministic, seed free.

The controller emits a ``(n_worlds, steps, 42)`` float32 target table on the GPU, i.e. exactly the input of
``HIPSimulation.step_replay`` / ``nmf_step_replay``: the CPG runs inside the stepping kernel's control-load stage.

Leg adhesion driven by the gait (BASELINE config 5): ``stance_bins`` marks, per leg, the part of the step cycle in
which the claw is near its lowest point (forward kinematics of the cycle in the thorax frame); with
``adhesion=(stance, on, off)`` the table gets six more columns holding the adhesion control ``on`` in stance and
``off`` in swing.  The reference clamps adhesion controls to [1, 100] (``compose/fly.py:434-440``), so "off" is 1.

``TurningCPG`` makes the same gait a small recurrent system that is advanced on the device between physics launches
(``csrc/nmf_cpg.hip``; specification ``tests/cpg_spec.py``; build-defined like ``TripodCPG``, in the form of flygym 1.x's
turning controller): six coupled phase oscillators per world with a phase (cycles, float64) and a magnitude each, and a per-world
drive ``(d_left, d_right)`` — ``|d|`` is the magnitude a side's legs converge to, ``sign(d)`` the direction its phases run in.
With the unit drive it reproduces ``TripodCPG.targets``; a weaker side shortens that side's strides and the fly turns towards it.

``HybridTurningCPG`` is that CPG plus the rule half of flygym 1.x's hybrid controller (specification ``tests/hybrid_spec.py``;
build-defined and pinned by nothing: the rules are this project's statement of them, the default constants flygym 1.x's as
remembered): a leg that hangs much lower than the others (it stepped into a gap) and a leg that is pushed backwards
while it swings (it hit a wall) are lifted by a correction added to their targets.  The rules read the batch's pose and contact
sensors once per launch; the oscillators are not changed by them.

``RuleBasedController`` is flygym 1.x's third walking controller, the decentralised one: no oscillators, every leg starts a step
when Cruse's rules 1 to 3 — scored from the other legs' step counters — say so, and the gait follows from the weights
(``csrc/nmf_rules.hip``; specification ``tests/rules_spec.py``; build-defined and pinned by nothing).  It takes the
same drive and writes the same table as ``TurningCPG``.

``SensorySteering`` closes the loop from the senses: one stateless launch (``csrc/nmf_taxis.hip``; specification
``tests/taxis_spec.py``) turns the ommatidia readings of both eyes and the readings of the four odor sites into the drive of a
``TurningCPG`` — flygym 1.x's visual taxis and odor taxis, build-defined and pinned by nothing.

``PlumeNavigator`` steers the CPG through an intermittent plume: a stochastic walk / stop / turn state machine per world, driven by
odor onsets and biased upwind, with its state and its noise counter on the device (``csrc/nmf_navigator.hip``; specification
``tests/navigator_spec.py``) — the navigator of flygym 1.x's plume-tracking task, build-defined and pinned by nothing.

``HeadStabilizer`` drives the neck from a small network: per world an MLP from the leg joint angles and the leg contact flags to
the neck's roll and pitch, evaluated in one stateless launch that writes ``ctrl`` (``csrc/nmf_stabilizer.hip``; specification
``tests/stabilizer_spec.py``) — flygym 1.x's head stabilization, build-defined and pinned by nothing.  The CPGs
take the leg dofs among a fly's position actuators as their columns, so a fly whose neck is actuated can walk under them.
"""

from __future__ import annotations

import ctypes

import numpy as np

from . import _native
from ._handle import NativeHandle, _field_view, check_params, fly_batch, leg_segments, reset_mask
from .anatomy import LEGS, JointDOF
from .replay import MotionSnippet

__all__ = ["TripodCPG", "TurningCPG", "HybridTurningCPG", "RuleBasedController", "rule_matrices", "swing_runs", "SensorySteering", "PlumeNavigator", "navigator_constants", "HeadStabilizer", "NECK_DOFS",
           "LEVELLING_NECK_DOFS"]

TRIPOD_PHASE_BIAS = {"lf": 0.0, "rm": 0.0, "lh": 0.0, "rf": np.pi, "lm": np.pi, "rh": np.pi}


class TripodCPG:
    def __init__(self, actuated_dofs: list[JointDOF], timestep: float, *, frequency: float = 12.0, n_phase_bins: int = 256):
        # the columns are the leg dofs of the list: a fly with a neck may carry position actuators on other joints (the head's, for
        # :class:`HeadStabilizer`), which the walking clip does not drive
        given = list(actuated_dofs)
        self.leg_columns = np.array([i for i, d in enumerate(given) if d.child.pos in LEGS], dtype=np.int64)
        self.n_given = len(given)
        self.actuated_dofs = [given[i] for i in self.leg_columns]
        self.timestep = float(timestep)
        self.frequency = float(frequency)
        self.n_bins = int(n_phase_bins)
        # (T, n) at the sim timestep.  Dofs the walking clip does not have (ALL_POSSIBLE's extra axes of the leg joints) are
        # held at zero, their neutral angle.
        snippet = MotionSnippet()
        in_clip = [(d.parent.link, d.child.link, d.axis.value) in snippet.dofs_per_leg for d in self.actuated_dofs]
        known = [d for d, k in zip(self.actuated_dofs, in_clip) if k]
        part = snippet.get_joint_angles(timestep, known)
        clip = np.zeros((part.shape[0], len(self.actuated_dofs)), dtype=part.dtype)
        clip[:, np.nonzero(in_clip)[0]] = part
        self.leg_of_dof = np.array([LEGS.index(d.child.pos) for d in self.actuated_dofs])
        self.cycle = np.zeros((self.n_bins, len(self.actuated_dofs)), dtype=np.float32)
        for leg in range(6):
            cols = np.where(self.leg_of_dof == leg)[0]
            knee = [i for i, c in enumerate(cols) if (self.actuated_dofs[c].parent.link, self.actuated_dofs[c].child.link,
                                                      self.actuated_dofs[c].axis.value) == ("trochanterfemur", "tibia", "pitch")]
            self.cycle[:, cols] = self._step_cycle(clip[:, cols], knee[0] if knee else min(5, len(cols) - 1))

    def _step_cycle(self, angles: np.ndarray, key_col: int) -> np.ndarray:
        """One periodic stride of a leg: stance/swing onsets from the trochanterfemur-tibia pitch angle's
        upward mean crossings, strides resampled to ``n_bins`` phase bins and averaged."""
        key = angles[:, key_col]
        centred = key - key.mean()
        onsets = np.where((centred[:-1] < 0) & (centred[1:] >= 0))[0]
        onsets = onsets[np.diff(onsets, prepend=-10 ** 9) > int(0.02 / self.timestep)]   # debounce 20 ms
        grid = np.linspace(0.0, 1.0, self.n_bins, endpoint=False)
        strides = []
        for a, b in zip(onsets[:-1], onsets[1:]):
            if b - a < int(0.03 / self.timestep):
                continue
            src = np.linspace(0.0, 1.0, b - a, endpoint=False)
            strides.append(np.stack([np.interp(grid, src, angles[a:b, k]) for k in range(angles.shape[1])], axis=1))
        if not strides:
            raise ValueError("no stride found in the clip")
        cyc = np.mean(strides, axis=0)
        # make the cycle periodic: remove the end-to-start jump linearly over the cycle
        jump = cyc[0] - (2 * cyc[-1] - cyc[-2])
        cyc = cyc + np.outer(grid, jump)
        return cyc.astype(np.float32)

    def phases(self, n_worlds: int, steps: int, start_step: int = 0, first_world: int = 0,
               total_worlds: int | None = None) -> np.ndarray:
        """(n_worlds, steps, 6) oscillator phases in [0, 2 pi); ``first_world`` / ``total_worlds`` place a
        shard of worlds inside a larger (multi-GPU) population."""
        t = (start_step + np.arange(steps)) * self.timestep
        world = 2 * np.pi * (first_world + np.arange(n_worlds)) / (total_worlds or n_worlds)
        bias = np.array([TRIPOD_PHASE_BIAS[leg] for leg in LEGS])
        ph = 2 * np.pi * self.frequency * t[None, :, None] + world[:, None, None] + bias[None, None, :]
        return np.mod(ph, 2 * np.pi)

    def stance_bins(self, model, fly, threshold: float = 0.3) -> np.ndarray:
        """``(n_bins, 6)`` bool: leg ``l`` is in stance in phase bin ``i`` when the origin of its last tarsal segment,
        computed by forward kinematics of the step cycle with the thorax at the identity pose, lies within
        ``threshold`` of its height range above its lowest point.  ``model`` is the compiled model of a world
        holding ``fly`` (``HIPSimulation.model``)."""
        from .compiler.rigid import forward_kinematics

        pos_ids = [i for i, a in enumerate(fly.actuators) if a["kind"] == "position" and a["jointdof"].child.pos in LEGS]
        if len(pos_ids) != len(self.actuated_dofs):
            raise ValueError("the fly's position actuators do not match the controller's actuated dofs")
        qadr = np.asarray(model["act_trn"])[pos_ids] + 1
        segs = [s.name for s in fly.get_bodysegs_order()]
        claw_body = [int(model["seg_body"][segs.index(f"{leg}_tarsus5")]) for leg in LEGS]
        q = np.array(model["key_qpos"], dtype=np.float64)
        q[:7] = (0, 0, 0, 1, 0, 0, 0)
        z = np.zeros((self.n_bins, 6))
        for i in range(self.n_bins):
            q[qadr] = self.cycle[i]
            xpos, _, _ = forward_kinematics(model, q)
            z[i] = xpos[claw_body, 2]
        lo, hi = z.min(axis=0), z.max(axis=0)
        return z <= lo + threshold * (hi - lo)

    def targets(self, n_worlds: int, steps: int, start_step: int = 0, device=None, first_world: int = 0,
                total_worlds: int | None = None, adhesion=None):
        """Target table ``(n_worlds, steps, n_act)`` float32: a torch tensor built on ``device`` if given (no large
        host arrays), else numpy.  ``adhesion=(stance_bins, on, off)`` appends six adhesion-control columns
        (legs in ``LEGS`` order): ``on`` while the leg's phase bin is a stance bin, else ``off``."""
        if adhesion is not None:
            stance, on, off = adhesion
            pos = self.targets(n_worlds, steps, start_step, device, first_world, total_worlds)
            legbias = np.array([TRIPOD_PHASE_BIAS[leg] for leg in LEGS])
            if device is None:
                ph = self.phases(n_worlds, steps, start_step, first_world, total_worlds)
                idx = np.floor(ph / (2 * np.pi) * self.n_bins).astype(np.int64) % self.n_bins
                adh = np.where(np.asarray(stance)[idx, np.arange(6)[None, None, :]], on, off).astype(np.float32)
                return np.ascontiguousarray(np.concatenate([pos, adh], axis=2))
            import torch

            st = torch.as_tensor(np.asarray(stance), device=device)
            t = (start_step + torch.arange(steps, device=device, dtype=torch.float64)) * self.timestep * self.frequency
            w = (first_world + torch.arange(n_worlds, device=device, dtype=torch.float64)) / float(total_worlds or n_worlds)
            b = torch.as_tensor(legbias / (2 * np.pi), device=device, dtype=torch.float64)
            x = torch.remainder(t[None, :, None] + w[:, None, None] + b[None, None, :], 1.0) * self.n_bins
            idx = torch.floor(x).to(torch.int64) % self.n_bins
            adh = torch.where(st[idx, torch.arange(6, device=device)[None, None, :]],
                              torch.tensor(float(on), device=device), torch.tensor(float(off), device=device))
            return torch.cat([pos, adh.to(torch.float32)], dim=2).contiguous()
        n_act = len(self.actuated_dofs)
        bias = np.array([TRIPOD_PHASE_BIAS[leg] for leg in LEGS])[self.leg_of_dof]                 # (n_act,)
        if device is None:
            ph = self.phases(n_worlds, steps, start_step, first_world, total_worlds)[..., self.leg_of_dof]
            x = ph / (2 * np.pi) * self.n_bins
            i0 = np.floor(x).astype(np.int64) % self.n_bins
            frac = (x - np.floor(x)).astype(np.float32)
            cols = np.arange(n_act)[None, None, :]
            table = (1 - frac) * self.cycle[i0, cols] + frac * self.cycle[(i0 + 1) % self.n_bins, cols]
            return np.ascontiguousarray(table.astype(np.float32))
        import torch

        # phase in cycles, float64 on the device for the same rounding as the numpy path, world chunks bound memory
        cyc = torch.as_tensor(self.cycle, device=device)                                            # (bins, n_act)
        t = (start_step + torch.arange(steps, device=device, dtype=torch.float64)) * self.timestep * self.frequency
        b = torch.as_tensor(bias / (2 * np.pi), device=device, dtype=torch.float64)
        out = torch.empty((n_worlds, steps, n_act), dtype=torch.float32, device=device)
        cols = torch.arange(n_act, device=device)[None, None, :]
        chunk = max(1, (1 << 24) // max(1, steps * n_act))
        for w0 in range(0, n_worlds, chunk):
            w = torch.arange(w0, min(n_worlds, w0 + chunk), device=device, dtype=torch.float64)
            world = (first_world + w) / float(total_worlds or n_worlds)
            x = torch.remainder(t[None, :, None] + world[:, None, None] + b[None, None, :], 1.0) * self.n_bins
            i0 = torch.floor(x).to(torch.int64) % self.n_bins
            frac = (x - torch.floor(x)).to(torch.float32)
            out[w0:w0 + len(w)] = (1 - frac) * cyc[i0, cols] + frac * cyc[(i0 + 1) % self.n_bins, cols]
        return out


STUMBLING_DEFAULT = 5.2          # force units: 1.25 x the most negative push of a swinging leg in flat walking (profiles/hybrid_cpg.txt)


class _CpgParams(ctypes.Structure):
    """``nmf_cpg_params`` of include/nmf.h."""

    _fields_ = [("n_pos", ctypes.c_int32), ("n_bins", ctypes.c_int32), ("frequency", ctypes.c_double), ("timestep", ctypes.c_double),
                ("coupling", ctypes.c_float), ("convergence", ctypes.c_float), ("adhesion_on", ctypes.c_float),
                ("adhesion_off", ctypes.c_float), ("table_steps", ctypes.c_int32)]


def _table_columns(cpg: TripodCPG, sim, fly_name: str, with_adhesion: bool):
    """``(act_ids, n_act)`` of the table a controller built on ``cpg`` writes for ``fly_name``: the ctrl ids of its leg columns (and
    of the six adhesion columns) and their number."""
    act_ids = sim.replay_ids(fly_name, with_adhesion=with_adhesion)
    if len(cpg.leg_columns) != cpg.n_given:              # position actuators off the legs: their ctrl columns are not the table's
        keep = [*cpg.leg_columns.tolist(), *range(cpg.n_given, int(act_ids.numel()))]
        act_ids = act_ids[sim._torch.as_tensor(keep, device=sim.device)].contiguous()
    n_act = len(cpg.actuated_dofs) + (6 if with_adhesion else 0)
    if int(act_ids.numel()) != n_act:
        raise ValueError(f"the fly has {int(act_ids.numel())} actuators for a table of {n_act} columns")
    return act_ids, n_act


class TurningCPG(NativeHandle, TripodCPG):
    """Closed-loop tripod CPG of one fly of a :class:`~flygym_amd.HIPSimulation`, advanced on the GPU (``nmf_cpg_advance``).

    Per step and world (every right-hand side from the old state; the row is computed before the update)::

        theta_l <- (theta_l + dt (frequency sign(d_side) + (1 / 2 pi) sum_{j != l} r_j coupling sin(2 pi (theta_j - theta_l) - (b_j - b_l)))) mod 1
        r_l     <- r_l + dt convergence (|d_side| - r_l)
        target[col] = c + (r_l - 1) (c - mean[col]),  c = the step cycle interpolated at theta_l

    Args:
        sim: the batch; for a world with several flies ``sim.for_fly(fly_name)``.
        fly_name: the fly whose position (and adhesion) actuators the table drives.
        frequency, coupling, convergence, n_phase_bins: the shared parameters.
        adhesion: ``(on, off)`` or ``(on, off, threshold)`` appends six adhesion columns that follow ``stance_bins``.
        table_steps: rows per world of the controller's own table: the most steps of one :meth:`advance`.

    ``phase`` ``(n, 6)`` float64, ``magnitude`` ``(n, 6)`` float32 and ``drive`` ``(n, 2)`` float32 are zero-copy views of the
    device state, writable between launches.  A new controller is reset: the tripod, world ``w`` at the phase offset ``w / n``.
    """

    _advance_entry = "nmf_cpg_advance"                   # the library entry point behind :meth:`advance`
    _destroy_entry, _noun, _views = "nmf_cpg_destroy", "controller", ("phase", "magnitude", "drive")

    def __init__(self, sim, fly_name: str, *, frequency: float = 12.0, coupling: float = 10.0, convergence: float = 20.0,
                 n_phase_bins: int = 256, adhesion=None, table_steps: int = 64):
        sim = fly_batch(sim, fly_name, resolve=False)
        if fly_name not in sim.world.fly_lookup:
            raise ValueError(f"no fly named {fly_name!r} in this simulation ({', '.join(sim.world.fly_lookup)})")
        if int(table_steps) < 1:
            raise ValueError(f"table_steps must be at least 1, got {table_steps}")
        if int(n_phase_bins) < 2:
            raise ValueError(f"n_phase_bins must be at least 2, got {n_phase_bins}")
        fly = sim.world.fly_lookup[fly_name]
        super().__init__(fly.get_actuated_jointdofs_order("position"), sim.timestep, frequency=frequency, n_phase_bins=n_phase_bins)
        self.sim, self.fly_name = sim, fly_name
        self.coupling, self.convergence = float(coupling), float(convergence)
        self.n_worlds, self.table_steps = int(sim.n_worlds), int(table_steps)
        self.adhesion, self.stance = None, None
        if adhesion is not None:
            if len(adhesion) not in (2, 3):
                raise ValueError(f"adhesion must be (on, off) or (on, off, threshold), got {adhesion!r}")
            self.adhesion = (float(adhesion[0]), float(adhesion[1]))
            self.stance = self.stance_bins(sim.model, fly, *([float(adhesion[2])] if len(adhesion) == 3 else []))
        self.act_ids, self.n_act = _table_columns(self, sim, fly_name, adhesion is not None)
        n_pos = len(self.actuated_dofs)
        check_params(_CpgParams, "nmf_cpg_params_size", "controllers.py")
        on, off = self.adhesion or (0.0, 0.0)
        self._params = _CpgParams(n_pos, self.n_bins, self.frequency, self.timestep, self.coupling, self.convergence, on, off,
                                  self.table_steps)
        cycle = np.ascontiguousarray(self.cycle, dtype=np.float32)
        legs = np.ascontiguousarray(self.leg_of_dof, dtype=np.int32)
        stance = None if self.stance is None else np.ascontiguousarray(self.stance, dtype=np.uint8)
        self._create("nmf_cpg_create", sim._batch_h, ctypes.byref(self._params), cycle.ctypes.data, legs.ctypes.data,
                     None if stance is None else stance.ctypes.data)
        self.phase, self.magnitude, self.drive = (_field_view(sim, _native.lib().nmf_cpg_field_ptr, self._h, which, typestr)
                                                  for which, typestr in ((0, "<f8"), (1, "<f4"), (2, "<f4")))
        t = sim._torch
        self.table = t.zeros((self.n_worlds, self.table_steps, self.n_act), dtype=t.float32, device=sim.device)

    # ---- control
    def set_drive(self, drive) -> None:
        """``(n_worlds, 2)`` (left, right), numpy or torch: copied into :attr:`drive` on the simulation's stream."""
        self._handle()
        t = self.sim._torch
        if not isinstance(drive, t.Tensor):
            drive = t.as_tensor(np.array(drive, dtype=np.float32))
        if tuple(drive.shape) != (self.n_worlds, 2):
            raise ValueError(f"Expected a drive of shape ({self.n_worlds}, 2), but got {tuple(drive.shape)}")
        self.drive.copy_(drive.to(device=self.sim.device, dtype=t.float32))

    def reset(self, mask=None, first_world: int = 0, total_worlds: int | None = None) -> None:
        """The worlds of ``mask`` (``(n_worlds,)`` bool, numpy or torch; default all) go back to the tripod with
        ``theta_l = ((first_world + w) / total_worlds + b_l / 2 pi) mod 1``, ``r = 1``, ``drive = (1, 1)``; the others keep their
        state.  Stream-ordered device work (no host sync)."""
        h = self._handle()
        total = self.n_worlds if total_worlds is None else int(total_worlds)
        if int(first_world) < 0 or int(first_world) + self.n_worlds > total:
            raise ValueError(f"worlds {first_world}..{int(first_world) + self.n_worlds - 1} do not lie inside a population of {total}")
        m = reset_mask(mask, self.n_worlds, self.sim)
        _native.check(_native.lib().nmf_cpg_reset(h, None if m is None else m.data_ptr(), int(first_world), total, self.sim._stream()))

    def advance(self, n_steps: int):
        """Advance every world by ``n_steps`` (1..table_steps) in one launch and write rows ``0 .. n_steps - 1`` of the
        controller's table; returns the table ``(n_worlds, table_steps, n_act)`` (a view: the next call overwrites it)."""
        h = self._handle()
        n = int(n_steps)
        if not 1 <= n <= self.table_steps:
            raise ValueError(f"n_steps must be in 1..{self.table_steps} (table_steps), got {n_steps}")
        advance = getattr(_native.lib(), self._advance_entry)
        _native.check(advance(h, n, self.table.data_ptr(), self.table_steps, self.sim._stream()))
        return self.table

    def step(self, n_steps: int, record_every: int | None = None):
        """One control tick: :meth:`advance`, then ``sim.step_replay`` over the rows just written (returns its observation
        ring when ``record_every`` is given)."""
        table = self.advance(n_steps)
        return self.sim.step_replay(table, self.act_ids, 0, int(n_steps), record_every)


class _CpgHybridParams(ctypes.Structure):
    """``nmf_cpg_hybrid_params`` of include/nmf.h."""

    _fields_ = [("retraction_threshold", ctypes.c_float), ("stumbling_force_threshold", ctypes.c_float),
                ("retraction_up", ctypes.c_float), ("retraction_down", ctypes.c_float), ("stumbling_up", ctypes.c_float),
                ("stumbling_down", ctypes.c_float), ("max_correction", ctypes.c_float)]


# Radians per unit of net correction over the seven leg dofs in the walking clip's order (coxa pitch, roll, yaw, femur pitch, roll,
# tibia pitch, tarsus pitch), by leg position: flygym 1.x's vectors as remembered.  The clip's angles are anatomical (a right leg
# mirrors its left one), so one vector serves both sides.
CORRECTION_VECTORS = {"f": (-0.03, 0.0, 0.0, -0.03, 0.0, 0.03, 0.03), "m": (-0.015, 0.001, 0.025, -0.02, 0.0, -0.02, 0.0),
                      "h": (0.0, 0.0, 0.0, -0.02, 0.0, 0.01, -0.02)}


class HybridTurningCPG(TurningCPG):
    """:class:`TurningCPG` plus the retraction and stumbling rules, advanced on the GPU (``nmf_cpg_advance_hybrid``).

    Decided once per launch, from the batch's ``seg_xpos`` / ``seg_xquat`` / ``sensordata`` as they stand when it starts (the last
    step of the previous tick; with ``advance(1)`` this is flygym 1.x's per-step rule)::

        h_l = z(root segment) - z(origin of {leg}_tarsus5);  L = argmax h (ties: the lowest index);  h3 = the third largest h
        retract[L] = h_L > h3 + retraction_threshold                                   (at most one leg per world)
        stumble[l] = leg l swings (the complement of stance_bins at its phase) and found_l > 0 and F_l . xhat < -stumbling_force_threshold

    with ``xhat`` the root segment's x axis and ``F_l`` the leg's net sensor force, both in the world frame.  Per step, the flags
    held for the launch and the row computed from the state before its update::

        net_l = rho_l > 0 ? rho_l : sigma_l
        target[col] = target of the CPG + net_l corr[col]          adhesion[l] = off while net_l > 0
        rho_l   <- retract[l] ? min(rho_l + dt up_r, max_correction)   : max(rho_l - dt down_r, 0)
        sigma_l <- stumble[l] ? min(sigma_l + dt up_s, max_correction) : max(sigma_l - dt down_s, 0)

    Args (beside :class:`TurningCPG`'s; the defaults are flygym 1.x's as remembered, the two thresholds measured on this model,
    ``profiles/hybrid_cpg.txt``):
        retraction_threshold: in the model's length unit.
        stumbling_force_threshold: in the contact sensors' force unit.
        retraction_rates, stumbling_rates: ``(up, down)`` per second.
        max_correction: the cap of ``rho`` and ``sigma``.
        correction_vectors: ``{"f": ..., "m": ..., "h": ...}``, seven values each over the leg dofs in the walking clip's order;
            columns of dofs outside the clip get 0.

    ``retraction`` and ``stumbling`` ``(n, 6)`` float32 and ``rule_flags`` ``(n, 6)`` uint8 (bit 0 retract, bit 1 stumble: the last
    launch's decision) are zero-copy views; :meth:`reset` clears them for the masked worlds.  :meth:`advance` is
    :meth:`TurningCPG.advance` with the rules: the launch decides from the batch's current pose and sensor outputs, writes
    :attr:`rule_flags` and advances :attr:`retraction` / :attr:`stumbling` with the oscillators.
    """

    _advance_entry = "nmf_cpg_advance_hybrid"
    _views = TurningCPG._views + ("retraction", "stumbling", "rule_flags")

    def __init__(self, sim, fly_name: str, *, retraction_threshold: float = 0.05, stumbling_force_threshold: float = STUMBLING_DEFAULT,
                 retraction_rates=(800.0, 700.0), stumbling_rates=(2200.0, 1800.0), max_correction: float = 80.0,
                 correction_vectors=None, **kw):
        super().__init__(sim, fly_name, **kw)
        try:
            self._enable(retraction_threshold, stumbling_force_threshold, retraction_rates, stumbling_rates, max_correction,
                         correction_vectors)
        except Exception:
            self.close()
            raise

    @staticmethod
    def correction_row(actuated_dofs, correction_vectors=None) -> np.ndarray:
        """``corr[n_pos]`` float32 for the columns ``actuated_dofs``: the vector of the leg's position at the dof's place in the
        walking clip's order, 0 for a dof the clip does not have."""
        vectors = dict(CORRECTION_VECTORS, **(correction_vectors or {}))
        clip_dofs = MotionSnippet().dofs_per_leg
        for key, vec in vectors.items():
            if key not in CORRECTION_VECTORS or len(vec) != len(clip_dofs):
                raise ValueError(f"correction_vectors takes {len(clip_dofs)} values for each of 'f', 'm', 'h', got {key!r}: {vec!r}")
        corr = np.zeros(len(actuated_dofs), dtype=np.float32)
        for c, d in enumerate(actuated_dofs):
            key = (d.parent.link, d.child.link, d.axis.value)
            if key in clip_dofs:
                corr[c] = vectors[d.child.pos[1]][clip_dofs.index(key)]
        return corr

    def _enable(self, retraction_threshold, stumbling_force_threshold, retraction_rates, stumbling_rates, max_correction,
                correction_vectors):
        sim, lib = self.sim, _native.lib()
        fly = sim.world.fly_lookup[self.fly_name]
        if len(retraction_rates) != 2 or len(stumbling_rates) != 2:
            raise ValueError("retraction_rates and stumbling_rates are (up, down) pairs")
        self.retraction_threshold, self.stumbling_force_threshold = float(retraction_threshold), float(stumbling_force_threshold)
        self.retraction_rates = (float(retraction_rates[0]), float(retraction_rates[1]))
        self.stumbling_rates = (float(stumbling_rates[0]), float(stumbling_rates[1]))
        self.max_correction = float(max_correction)
        self.corr = self.correction_row(self.actuated_dofs, correction_vectors)
        # swing: the complement of the stance bins, whether or not the table has adhesion columns
        stance = self.stance if self.stance is not None else self.stance_bins(sim.model, fly)
        self.swing = np.ascontiguousarray(~np.asarray(stance, dtype=bool), dtype=np.uint8)
        self.root_seg, self.tip_seg = leg_segments(fly, LEGS)
        check_params(_CpgHybridParams, "nmf_cpg_hybrid_params_size", "controllers.py")
        self._hybrid_params = _CpgHybridParams(self.retraction_threshold, self.stumbling_force_threshold, *self.retraction_rates,
                                               *self.stumbling_rates, self.max_correction)
        _native.check(lib.nmf_cpg_hybrid_enable(self._h, ctypes.byref(self._hybrid_params), self.corr.ctypes.data,
                                                self.swing.ctypes.data, self.root_seg, self.tip_seg.ctypes.data))
        self.retraction, self.stumbling, self.rule_flags = (_field_view(sim, lib.nmf_cpg_field_ptr, self._h, which, typestr)
                                                            for which, typestr in ((3, "<f4"), (4, "<f4"), (5, "|u1")))


RULE_NAMES = ("rule1", "rule2_ipsi", "rule2_contra", "rule3_ipsi", "rule3_contra")
RULE_WEIGHTS = {"rule1": -10.0, "rule2_ipsi": 2.5, "rule2_contra": 1.0, "rule3_ipsi": 3.0, "rule3_contra": 2.0}


def default_rules_graph() -> dict:
    """``{rule name: [(source leg, target leg), ...]}``: rule 1 from a leg to its posterior neighbour, rule 2 from a leg to its
    anterior neighbour and both ways across each contralateral pair, rule 3 from a leg to its posterior neighbour and both ways
    across each contralateral pair."""
    backwards = [(f"{side}{a}", f"{side}{b}") for side in "lr" for a, b in ("fm", "mh")]
    across = [(f"{a}{pos}", f"{b}{pos}") for pos in "fmh" for a, b in ("lr", "rl")]
    return {"rule1": backwards, "rule2_ipsi": [(b, a) for a, b in backwards], "rule2_contra": across, "rule3_ipsi": backwards,
            "rule3_contra": across}


def rule_matrices(rules_graph=None, weights=None) -> np.ndarray:
    """``(3, 6, 6)`` float32 ``[rule][source][target]``, legs in ``LEGS`` order: the matrices W1, W2, W3 of
    :class:`RuleBasedController`.  ``rules_graph`` replaces the edge lists of the rule names it holds in
    :func:`default_rules_graph`, ``weights`` the values it holds in ``RULE_WEIGHTS``; an edge listed under both names of a rule
    gets the sum.  Needs no GPU."""
    graph, values = default_rules_graph(), dict(RULE_WEIGHTS)
    for name, given, known in (("rules_graph", rules_graph, graph), ("weights", weights, values)):
        for key, value in (given or {}).items():
            if key not in RULE_NAMES:
                raise ValueError(f"{name} takes the keys {', '.join(RULE_NAMES)}, got {key!r}")
            known[key] = value
    out = np.zeros((3, 6, 6), dtype=np.float32)
    for key in RULE_NAMES:
        weight = float(values[key])
        if not np.isfinite(weight):
            raise ValueError(f"the weight of {key} is not finite: {values[key]!r}")
        for edge in graph[key]:
            if len(edge) != 2 or edge[0] not in LEGS or edge[1] not in LEGS:
                raise ValueError(f"an edge of {key} is a pair of legs out of {', '.join(LEGS)}, got {edge!r}")
            out[int(key[4]) - 1, LEGS.index(edge[0]), LEGS.index(edge[1])] += np.float32(weight)
    return out


def swing_runs(stance) -> tuple:
    """``(start_bin[6], swing_bins[6])`` int32 of a stance table ``(n_bins, 6)``: per leg the first bin and the length of the longest
    circular run of swing bins (the bins that are not stance); of runs of equal length the one that starts at the lowest bin.  A leg
    whose bins are all swing or all stance raises ``ValueError``.  Needs no GPU."""
    swing = ~np.asarray(stance, dtype=bool)
    if swing.ndim != 2 or swing.shape[1] != 6 or swing.shape[0] < 2:
        raise ValueError(f"a stance table is (n_bins >= 2, 6), got {swing.shape}")
    n = swing.shape[0]
    start, length = np.zeros(6, dtype=np.int32), np.zeros(6, dtype=np.int32)
    for leg in range(6):
        col = swing[:, leg]
        if col.all() or not col.any():
            raise ValueError(f"leg {LEGS[leg]} is in {'swing' if col.all() else 'stance'} in every bin")
        for b in range(n):
            if col[b] and not col[b - 1]:                # a run starts here (bin -1 is the last one)
                run = 1
                while col[(b + run) % n]:
                    run += 1
                if run > length[leg]:
                    start[leg], length[leg] = b, run
    return start, length


class _RulesParams(ctypes.Structure):
    """``nmf_rules_params`` of include/nmf.h."""

    _fields_ = [("n_pos", ctypes.c_int32), ("n_bins", ctypes.c_int32), ("period_steps", ctypes.c_int32), ("table_steps", ctypes.c_int32),
                ("adhesion", ctypes.c_int32), ("adhesion_on", ctypes.c_float), ("adhesion_off", ctypes.c_float), ("margin", ctypes.c_float),
                ("max_amplitude", ctypes.c_float), ("seed", ctypes.c_uint32), ("first_world", ctypes.c_int32)]


class RuleBasedController(NativeHandle, TripodCPG):
    """Rule-based walking of one fly of a :class:`~flygym_amd.HIPSimulation`, advanced on the GPU (``nmf_rules_advance``,
    ``csrc/nmf_rules.hip``): every leg decides by Cruse's rules when to start a step, in the form of flygym 1.x's decentralised
    rule-based controller.  No gait is programmed; tripod, tetrapod and wave gaits follow from the weights.

    Build-defined and pinned by nothing (the reference ships no controllers; nothing is claimed about matching flygym 1.x): the rule
    graph and the weights are flygym 1.x's as remembered, the statement of the model is include/nmf.h (``nmf_rules_advance``), its
    specification in numpy tests/rules_spec.py.  Per leg a counter ``k`` in ``[0, P)``: 0 rests at the pose where the leg's swing
    starts, and a step runs the leg's cycle of :class:`TripodCPG` once in ``P`` physics steps, swing first.  Per physics step, from
    the six counters alone (the rules read neither the pose nor the contact sensors)::

        swinging_s = 0 < k_s < swing_steps[s];   p_s = max(0, k_s - swing_steps[s]) / (P - swing_steps[s])     (stance progress)
        score_t = sum_s swinging_s W1[s][t]  +  sum_{p_s > 0} W2[s][t] (1 - p_s)  +  sum_{p_s > 0} W3[s][t] p_s
        eligible_t = score_t > 0, within ``margin`` of the best score, not stepping, and drive[side_t] != 0
        nobody stepping and nobody eligible: every leg of a driven side is eligible       (the walk starts, or starts again)
        one eligible leg, drawn uniformly, starts a step with the amplitude a = min(|drive[side]|, max_amplitude)
        target[col] = rest + a (c - rest),  c = the step cycle interpolated at k / P,  rest = the cycle where the swing starts

    The draw is a counter-based hash of ``(seed, first_world + w, ticks[w])``, the plume's with a draw index of its own, so a
    world's walk does not depend on the batch it is stepped in and a captured tick draws afresh on every replay.

    Args:
        sim: the batch; for a world with several flies ``sim.for_fly(fly_name)``.
        fly_name: the fly whose position (and adhesion) actuators the table drives.
        frequency: steps of a leg per second; period_steps: ``P``, default ``round(1 / (frequency * timestep))``.
        n_phase_bins: bins of the step cycle.
        adhesion: ``(on, off)`` or ``(on, off, threshold)`` appends six adhesion columns: ``off`` while the leg swings.
        table_steps: rows per world of the controller's own table: the most steps of one :meth:`advance`.
        rules_graph, weights: see :func:`rule_matrices`.
        margin: a leg is eligible when its score is at least ``best - |best| * margin``.
        max_amplitude: the cap of a step's amplitude.
        seed, first_world: the draws; ``first_world`` places a shard of worlds inside a larger population.

    ``counter`` ``(n, 6)`` int32, ``stepping`` ``(n, 6)`` uint8, ``amplitude`` ``(n, 6)`` float32, ``drive`` ``(n, 2)`` float32,
    ``ticks`` ``(n,)`` (the device's uint32 counter seen as int32) and ``scores`` ``(n, 6)`` float32 (of the last step) are zero-copy
    views of the device state, writable between launches.  ``drive`` has the shape of ``TurningCPG.drive`` and its meaning of
    magnitude — ``SensorySteering.update(out=ctl.drive)`` and ``PlumeNavigator.update(..., out=ctl.drive)`` steer it unchanged —
    but the sign of a drive is ignored: legs only ever step forwards, and a side whose drive is 0 starts no step.  A new
    controller is reset: every leg at rest, drive ``(1, 1)``.
    """

    _advance_entry = "nmf_rules_advance"
    _destroy_entry, _noun = "nmf_rules_destroy", "controller"
    _views = ("counter", "stepping", "amplitude", "drive", "ticks", "scores")

    def __init__(self, sim, fly_name: str, *, frequency: float = 12.0, period_steps: int | None = None, n_phase_bins: int = 256,
                 adhesion=None, table_steps: int = 64, rules_graph=None, weights=None, margin: float = 1e-3, max_amplitude: float = 1.5,
                 seed: int = 0, first_world: int = 0):
        sim = fly_batch(sim, fly_name, resolve=False)
        if fly_name not in sim.world.fly_lookup:
            raise ValueError(f"no fly named {fly_name!r} in this simulation ({', '.join(sim.world.fly_lookup)})")
        if int(table_steps) < 1:
            raise ValueError(f"table_steps must be at least 1, got {table_steps}")
        if int(n_phase_bins) < 2:
            raise ValueError(f"n_phase_bins must be at least 2, got {n_phase_bins}")
        if period_steps is None:
            if not (np.isfinite(frequency) and frequency > 0):
                raise ValueError(f"frequency must be positive and finite, got {frequency!r}")
            period_steps = round(1.0 / (float(frequency) * float(sim.timestep)))
        period = int(period_steps)
        if period < 2 or period * int(n_phase_bins) >= 2 ** 31:
            raise ValueError(f"period_steps must be at least 2 with period_steps * n_phase_bins below 2^31, got {period} * {n_phase_bins}")
        if adhesion is not None and len(adhesion) not in (2, 3):
            raise ValueError(f"adhesion must be (on, off) or (on, off, threshold), got {adhesion!r}")
        for name, value in (("margin", margin), ("max_amplitude", max_amplitude)):
            if not (np.isfinite(value) and value >= 0):
                raise ValueError(f"{name} must be finite and not negative, got {value!r}")
        if int(first_world) < 0:
            raise ValueError(f"first_world must not be negative, got {first_world}")
        self.weights = rule_matrices(rules_graph, weights)
        fly = sim.world.fly_lookup[fly_name]
        super().__init__(fly.get_actuated_jointdofs_order("position"), sim.timestep, frequency=frequency, n_phase_bins=n_phase_bins)
        self.sim, self.fly_name = sim, fly_name
        self.n_worlds, self.table_steps, self.period_steps = int(sim.n_worlds), int(table_steps), period
        self.margin, self.max_amplitude = float(margin), float(max_amplitude)
        self.seed, self.first_world = int(seed) & 0xFFFFFFFF, int(first_world)
        self.adhesion = None if adhesion is None else (float(adhesion[0]), float(adhesion[1]))
        self.stance = self.stance_bins(sim.model, fly, *([float(adhesion[2])] if adhesion is not None and len(adhesion) == 3 else []))
        self.start_bin, self.swing_bins = swing_runs(self.stance)
        self.swing_steps = ((self.swing_bins.astype(np.int64) * period + self.n_bins - 1) // self.n_bins).astype(np.int32)
        if (self.swing_steps >= period).any():
            raise ValueError(f"a swing of {self.swing_steps.tolist()} steps leaves no stance in a period of {period} steps")
        self.act_ids, self.n_act = _table_columns(self, sim, fly_name, adhesion is not None)
        check_params(_RulesParams, "nmf_rules_params_size", "controllers.py")
        on, off = self.adhesion or (0.0, 0.0)
        self._params = _RulesParams(len(self.actuated_dofs), self.n_bins, period, self.table_steps, int(adhesion is not None), on, off,
                                    self.margin, self.max_amplitude, self.seed, self.first_world)
        cycle = np.ascontiguousarray(self.cycle, dtype=np.float32)
        legs = np.ascontiguousarray(self.leg_of_dof, dtype=np.int32)
        h = self._create("nmf_rules_create", sim._batch_h, ctypes.byref(self._params), cycle.ctypes.data, legs.ctypes.data,
                         self.start_bin.ctypes.data, self.swing_steps.ctypes.data, self.weights.ctypes.data)
        view = lambda which, typestr: _field_view(sim, _native.lib().nmf_rules_field_ptr, h, which, typestr)
        self.counter, self.stepping, self.amplitude = view(0, "<i4"), view(1, "|u1"), view(2, "<f4")
        self.drive, self.ticks, self.scores = view(3, "<f4"), view(4, "<i4").reshape(self.n_worlds), view(5, "<f4")
        t = sim._torch
        self.table = t.zeros((self.n_worlds, self.table_steps, self.n_act), dtype=t.float32, device=sim.device)

    # the drive, the launch and the control tick are TurningCPG's, word for word: both write the table nmf_step_replay reads
    set_drive, advance, step = TurningCPG.set_drive, TurningCPG.advance, TurningCPG.step

    def reset(self, mask=None) -> None:
        """The worlds of ``mask`` (``(n_worlds,)`` bool, numpy or torch; default all) start again: every leg at rest, amplitude 1,
        ``drive = (1, 1)``, tick 0 (their draws from the start), scores 0; the others keep their state.  Stream-ordered device work
        (no host sync)."""
        h = self._handle()
        m = reset_mask(mask, self.n_worlds, self.sim)
        _native.check(_native.lib().nmf_rules_reset(h, None if m is None else m.data_ptr(), self.sim._stream()))


class _TaxisParams(ctypes.Structure):
    """``nmf_taxis_params`` of include/nmf.h."""

    _fields_ = [("obj_threshold", ctypes.c_float), ("area_threshold", ctypes.c_float), ("visual_gain", ctypes.c_float),
                ("v_min", ctypes.c_float), ("v_max", ctypes.c_float), ("w_ant", ctypes.c_float), ("w_palp", ctypes.c_float),
                ("odor_delta", ctypes.c_float), ("base", ctypes.c_float), ("drive_min", ctypes.c_float), ("drive_max", ctypes.c_float),
                ("front_edge", ctypes.c_int32 * 2)]


def eye_front_edges() -> tuple:
    """Per eye of ``sensors.EYE_CAMERAS``: 1 when the fly's forward axis (+x of the eye's parent frame) has a positive component
    along the camera's right axis — column 0 of the camera matrix ``Rz Ry Rx`` of the eye's Euler triple — so that the image's
    LAST column faces forward; 0 when column 0 does.  (1, 0): left eye +0.892, right eye -0.892."""
    from .sensors import EYE_CAMERAS

    out = []
    for _, (_, e) in EYE_CAMERAS.items():
        # (Rz Ry Rx)[0, 0] = cos(e2) cos(e1)
        out.append(int(np.cos(e[2]) * np.cos(e[1]) > 0))
    return tuple(out)


class SensorySteering:
    """Eyes and antennae steer the CPG: one launch per control tick turns the ommatidia readings of both eyes
    (``EyeRenderer.render_into``) and the readings of the four odor sites (``OdorSensors`` / ``OdorPlume.get_odor_intensities``)
    into the drive ``(left, right)`` of a :class:`TurningCPG` (``nmf_taxis_update``, ``csrc/nmf_taxis.hip``; the model is stated in
    include/nmf.h and specified by tests/taxis_spec.py).  Stateless: no handle, nothing to close.

    Visual taxis (follow a dark object): an ommatidium is dark when its reading is below ``obj_threshold``; per eye ``area`` is the
    dark share of the ommatidia and ``(cx, cy)`` the mean centre of the dark ones in units of the image's width and height.  An eye
    has found the object when ``area > area_threshold``; its side's speed is then ``clip(1 - visual_gain * dev, v_min, v_max)``, ``dev``
    being the object's normalised distance from the image edge that faces forward (:attr:`front_edge`) — so the fly slows the
    side a lateral object is on and turns towards it — and 1 otherwise.

    Odor taxis: per odor dimension ``d`` the left and right readings are ``w_ant * antenna + w_palp * palp``, their contrast is
    ``c_d = (L - R) / (L + R)`` (0 without odor), ``b = sum_d odor_gains[d] * c_d`` (a positive gain attracts, a negative one
    repels), ``q = b |b| / (1 + b^2)``; the left speed is scaled by ``1 - odor_delta * max(q, 0)``, the right one by
    ``1 - odor_delta * max(-q, 0)``.

    ``drive[side] = clip(base * v_side * o_side, drive_min, drive_max)``, side 0 = left: the order of ``TurningCPG.drive``.  The
    defaults are flygym 1.x's constants as remembered (its source is not at hand); build-defined and pinned by nothing.

    Args:
        sim: the batch; a world with several flies resolves to ``sim.for_fly(fly_name)``.
        fly_name: the fly that is steered.
        retina: the retina whose readings :meth:`update` takes (default: the default :class:`~flygym_amd.sensors.Retina`); at most
            2047 pixels a side and 1024 ommatidia.
        odor_gains: one gain per odor dimension (at most 8).

    ``features`` ``(n, 2, 3)`` (cy, cx, area per eye), ``bias`` ``(n,)`` (the value ``b``) and ``drive`` ``(n, 2)`` are float32
    tensors allocated once and overwritten by every :meth:`update`.
    """

    def __init__(self, sim, fly_name: str, *, retina=None, odor_gains=(), obj_threshold: float = 0.15, area_threshold: float = 0.01,
                 visual_gain: float = 3.0, v_min: float = 0.4, v_max: float = 1.2, w_ant: float = 10.0 / 11.0, w_palp: float = 1.0 / 11.0,
                 odor_delta: float = 0.8, base: float = 1.0, drive_min: float = 0.2, drive_max: float = 1.2):
        from .sensors import Retina

        sim = fly_batch(sim, fly_name, resolve=True)
        if fly_name not in sim.world.fly_lookup:
            raise ValueError(f"no fly named {fly_name!r} in this simulation ({', '.join(sim.world.fly_lookup)})")
        self.sim, self.fly_name = sim, fly_name
        self.retina = retina or Retina()
        self.n_worlds, self.n_omm = int(sim.n_worlds), int(self.retina.num_ommatidia)
        table = self.retina.centre_table()                       # (refuses a retina the kernel's table cannot hold)
        self.odor_gains = tuple(float(g) for g in odor_gains)
        self.n_dims = len(self.odor_gains)
        if self.n_dims > 8:
            raise ValueError(f"at most 8 odor dimensions, got {self.n_dims} gains")
        self.front_edge = eye_front_edges()
        check_params(_TaxisParams, "nmf_taxis_params_size", "controllers.py")
        self._params = _TaxisParams(float(obj_threshold), float(area_threshold), float(visual_gain), float(v_min), float(v_max),
                                    float(w_ant), float(w_palp), float(odor_delta), float(base), float(drive_min), float(drive_max),
                                    (ctypes.c_int32 * 2)(*self.front_edge))
        t, dev = sim._torch, sim.device
        self.centres = t.as_tensor(table, device=dev)            # int16 (n_omm, 2), sixteenths of a pixel
        # (one element more than the gains: never empty, so its address also stands in for an odor input of no dimensions)
        self._gains = t.zeros((self.n_dims + 1,), dtype=t.float32, device=dev)
        if self.n_dims:
            self._gains[:self.n_dims] = t.as_tensor(np.array(self.odor_gains, dtype=np.float32), device=dev)
        self.features = t.zeros((self.n_worlds, 2, 3), dtype=t.float32, device=dev)
        self.bias = t.zeros((self.n_worlds,), dtype=t.float32, device=dev)
        self.drive = t.ones((self.n_worlds, 2), dtype=t.float32, device=dev)

    def _checked(self, name, x, shape):
        t = self.sim._torch
        if (not isinstance(x, t.Tensor) or tuple(x.shape) != shape or x.dtype != t.float32 or x.device != self.sim.device
                or not x.is_contiguous()):
            got = f"{tuple(x.shape)} {x.dtype} on {x.device}" if isinstance(x, t.Tensor) else type(x).__name__
            raise ValueError(f"{name} must be a contiguous float32 tensor of shape {shape} on {self.sim.device}, got {got}")
        return x

    def update(self, omm=None, odor=None, out=None):
        """One steering update from ``omm`` ``(n_worlds, 2, num_ommatidia, 2)`` and / or ``odor`` ``(n_worlds, n_dims, 4)`` (float32,
        contiguous, on the simulation's device): one kernel launch on the current stream, no allocation — capturable.  Writes
        :attr:`features` and :attr:`bias`, and the drive into ``out`` ``(n_worlds, 2)`` (for example ``cpg.drive``) or into
        :attr:`drive`; returns the drive tensor.  An absent input leaves its factor at 1."""
        n = self.n_worlds
        if omm is None and odor is None:
            raise ValueError("update needs omm, odor or both")
        if omm is not None:
            self._checked("omm", omm, (n, 2, self.n_omm, 2))
        odor_ptr = None
        if odor is not None:
            if isinstance(odor, self.sim._torch.Tensor) and odor.ndim == 3 and int(odor.shape[1]) != self.n_dims:
                raise ValueError(f"odor has {int(odor.shape[1])} dimensions for {self.n_dims} odor_gains")
            self._checked("odor", odor, (n, self.n_dims, 4))
            odor_ptr = odor.data_ptr() if self.n_dims else self._gains.data_ptr()
        drive = self.drive if out is None else self._checked("out", out, (n, 2))
        _native.check(_native.lib().nmf_taxis_update(
            ctypes.byref(self._params), self.centres.data_ptr(), self.n_omm, self.retina.height, self.retina.width,
            None if omm is None else omm.data_ptr(), odor_ptr, self._gains.data_ptr(), self.n_dims, n,
            self.features.data_ptr(), self.bias.data_ptr(), drive.data_ptr(), self.sim._stream()))
        return drive


class _NavigatorParams(ctypes.Structure):
    """``nmf_navigator_params`` of include/nmf.h."""

    _fields_ = [("seed", ctypes.c_uint32), ("first_world", ctypes.c_int32), ("root_seg", ctypes.c_int32), ("odor_dim", ctypes.c_int32),
                ("turn_ticks", ctypes.c_int32), ("dt", ctypes.c_float), ("threshold", ctypes.c_float), ("decay_stop", ctypes.c_float),
                ("decay_walk", ctypes.c_float), ("decay_freq", ctypes.c_float), ("inv_tau_freq", ctypes.c_float),
                ("lambda_ws0", ctypes.c_float), ("dlambda_ws", ctypes.c_float), ("lambda_sw0", ctypes.c_float),
                ("dlambda_sw", ctypes.c_float), ("lambda_turn", ctypes.c_float), ("p_up0", ctypes.c_float), ("up_gain", ctypes.c_float),
                ("p_up_min", ctypes.c_float), ("p_up_max", ctypes.c_float), ("walk_drive", ctypes.c_float * 2),
                ("stop_drive", ctypes.c_float * 2), ("turn_drive", ctypes.c_float * 2)]


def navigator_constants(tick_s: float, tau_stop: float, tau_walk: float, tau_freq: float, turn_duration: float) -> dict:
    """What :class:`PlumeNavigator` derives from its time constants, computed in float64 and rounded once to float32 — the kernel
    neither divides nor calls ``exp``: ``decay_x = exp(-tick_s / tau_x)``, ``inv_tau_freq = 1 / tau_freq`` and
    ``turn_ticks = round(turn_duration / tick_s)``."""
    dt = float(tick_s)
    taus = dict(stop=float(tau_stop), walk=float(tau_walk), freq=float(tau_freq))
    if not (np.isfinite(dt) and dt > 0):
        raise ValueError(f"tick_s must be positive and finite, got {tick_s!r}")
    for name, tau in taus.items():
        if not (np.isfinite(tau) and tau > 0):
            raise ValueError(f"tau_{name} must be positive and finite, got {tau!r}")
    if not np.isfinite(float(turn_duration)):
        raise ValueError(f"turn_duration must be finite, got {turn_duration!r}")
    out = {f"decay_{name}": np.float32(np.exp(-dt / tau)) for name, tau in taus.items()}
    out["inv_tau_freq"] = np.float32(1.0 / taus["freq"])
    out["turn_ticks"] = int(round(float(turn_duration) / dt))
    if not 1 <= out["turn_ticks"] <= 65535:
        raise ValueError(f"turn_duration / tick_s must round to 1..65535 ticks, got {out['turn_ticks']}")
    return out


class PlumeNavigator(NativeHandle):
    """Navigating an intermittent odor plume on the GPU (``nmf_navigator_*``): per world a stochastic walk / stop / turn state
    machine driven by odor onsets ("encounters"), in the form of Demir et al. 2020 as flygym 1.x steered its plume-tracking task
    with it, that writes the drive of a :class:`TurningCPG`.

    Build-defined and pinned by nothing (the reference ships no controllers; nothing is claimed about matching flygym 1.x); the
    statement of the model is include/nmf.h (``nmf_navigator_update``), its specification in numpy tests/navigator_spec.py.  One
    :meth:`update` per control tick, from the antennal readings, the wind and the root segment's attitude::

        e = the antennal sum I[2] + I[3] rose above ``threshold`` in this update                   (an encounter)
        k_stop <- k_stop decay_stop + e;  k_walk <- k_walk decay_walk + e;  freq <- freq decay_freq + e / tau_freq
        p_stop = clip(dt (stop_rate[0] + stop_rate[1] k_stop), 0, 1);  p_walk likewise from walk_rate and k_walk
        p_turn = clip(dt turn_rate, 0, 1);  p_up = clip(p_up[0] + p_up[1] freq, p_up_bounds)
        walking: stop with p_stop, else turn with p_turn for ``turn_duration`` — upwind with p_up, else downwind; stopped: walk with p_walk
        drive = walk_drive, stop_drive or turn_drive = (inner, outer) by the new state

    The three uniform draws of a tick are a counter-based hash of ``(seed, first_world + w, ticks[w])`` — the plume's, with its
    own draw indices —, so a world's decisions do not depend on the batch it is stepped in and a captured update draws fresh
    noise on every replay.

    Args:
        sim: the batch; for a world with several flies ``sim.for_fly(fly_name)``.
        fly_name: the fly that is steered (its root segment's attitude is read).
        tick_s: the control tick in seconds (one :meth:`update` per tick).
        threshold: of the antennal sum, in the readings' unit.
        seed, first_world: the noise streams; ``first_world`` places a shard of worlds inside a larger population.
        odor_dim: the odor dimension whose antennae are read (0..7).
        stop_rate, walk_rate: ``(base, change per unit of the filter)`` per second; turn_rate per second.
        tau_stop, tau_walk, tau_freq: the filters' time constants in seconds; turn_duration in seconds.
        p_up: ``(base, gain per unit of freq)``; p_up_bounds: ``(min, max)`` in [0, 1].
        walk_drive, stop_drive: ``(left, right)``; turn_drive: ``(inner, outer)``.

    The default rates and time constants are Demir et al.'s as flygym 1.x's tutorial used them, as remembered (its source is not at
    hand); the upwind probability is this project's linear stand-in for their sigmoid.  ``state`` (0 walk, 1 stop, 2 turn left,
    3 turn right), ``remaining``, ``encounters`` ``(n,)`` int32, ``above`` ``(n,)`` uint8, ``k_stop``, ``k_walk``, ``freq`` ``(n,)``
    float32, ``ticks`` ``(n,)`` (the device's uint32 counter seen as int32, as ``OdorPlume.ticks``) and ``drive`` ``(n, 2)`` float32 are zero-copy views of the device state, writable between
    launches.  Every method is stream-ordered device work on the simulation's stream; :meth:`update` is one launch and can be
    captured in a graph.  Close the navigator before its simulation.
    """

    WALK, STOP, TURN_LEFT, TURN_RIGHT = 0, 1, 2, 3
    _destroy_entry, _noun = "nmf_navigator_destroy", "navigator"
    _views = ("state", "remaining", "above", "k_stop", "k_walk", "freq", "ticks", "encounters", "drive")

    def __init__(self, sim, fly_name: str, *, tick_s: float, threshold: float, seed: int = 0, first_world: int = 0, odor_dim: int = 0,
                 stop_rate=(0.78, -0.61), walk_rate=(0.29, 0.41), turn_rate: float = 1.33, tau_stop: float = 0.2, tau_walk: float = 0.52,
                 tau_freq: float = 2.0, turn_duration: float = 0.25, p_up=(0.5, 0.15), p_up_bounds=(0.05, 0.95),
                 walk_drive=(1.0, 1.0), stop_drive=(0.0, 0.0), turn_drive=(-0.4, 1.2)):
        sim = fly_batch(sim, fly_name, resolve=False)
        if fly_name not in sim.world.fly_lookup:
            raise ValueError(f"no fly named {fly_name!r} in this simulation ({', '.join(sim.world.fly_lookup)})")
        for name, pair in (("stop_rate", stop_rate), ("walk_rate", walk_rate), ("p_up", p_up), ("p_up_bounds", p_up_bounds),
                           ("walk_drive", walk_drive), ("stop_drive", stop_drive), ("turn_drive", turn_drive)):
            if len(pair) != 2:
                raise ValueError(f"{name} takes two values, got {pair!r}")
        self.sim, self.fly_name = sim, fly_name
        self.n_worlds, self.tick_s = int(sim.n_worlds), float(tick_s)
        self.seed, self.first_world, self.odor_dim = int(seed) & 0xFFFFFFFF, int(first_world), int(odor_dim)
        self.constants = navigator_constants(tick_s, tau_stop, tau_walk, tau_freq, turn_duration)
        self.root_seg, _ = leg_segments(sim.world.fly_lookup[fly_name], LEGS)
        check_params(_NavigatorParams, "nmf_navigator_params_size", "controllers.py")
        pair = lambda v: (ctypes.c_float * 2)(float(v[0]), float(v[1]))
        c = self.constants
        self._params = _NavigatorParams(
            self.seed, self.first_world, self.root_seg, self.odor_dim, c["turn_ticks"], self.tick_s, float(threshold),
            float(c["decay_stop"]), float(c["decay_walk"]), float(c["decay_freq"]), float(c["inv_tau_freq"]), float(stop_rate[0]),
            float(stop_rate[1]), float(walk_rate[0]), float(walk_rate[1]), float(turn_rate), float(p_up[0]), float(p_up[1]),
            float(p_up_bounds[0]), float(p_up_bounds[1]), pair(walk_drive), pair(stop_drive), pair(turn_drive))
        h = self._create("nmf_navigator_create", sim._batch_h, ctypes.byref(self._params))
        view = lambda which, typestr: _field_view(sim, _native.lib().nmf_navigator_field_ptr, h, which, typestr)
        flat = lambda which, typestr: view(which, typestr).reshape(self.n_worlds)
        self.state, self.remaining, self.above = flat(0, "<i4"), flat(1, "<i4"), flat(2, "|u1")
        self.k_stop, self.k_walk, self.freq = flat(3, "<f4"), flat(4, "<f4"), flat(5, "<f4")
        self.ticks, self.encounters, self.drive = flat(6, "<i4"), flat(7, "<i4"), view(8, "<f4")

    def _checked(self, name, x, shapes):
        t = self.sim._torch
        if (not isinstance(x, t.Tensor) or tuple(x.shape) not in shapes or x.dtype != t.float32 or x.device != t.device(self.sim.device)
                or not x.is_contiguous()):
            got = f"{tuple(x.shape)} {x.dtype} on {x.device}" if isinstance(x, t.Tensor) else type(x).__name__
            raise ValueError(f"{name} must be a contiguous float32 tensor of shape {' or '.join(map(str, shapes))} on {self.sim.device}, "
                             f"got {got}")
        return x

    def update(self, odor, wind, out=None):
        """One update of every world from ``odor`` ``(n_worlds, n_dims, 4)`` (``OdorPlume.get_odor_intensities`` /
        ``OdorSensors``) and ``wind`` ``(n_worlds, 2)``, ``(1, 2)`` or ``(2,)`` (``OdorPlume.wind``; one row is shared by all
        worlds), float32, contiguous, on the simulation's device; the root segment's attitude is the batch's as it stands.  One
        kernel launch, no allocation — capturable.  Writes the drive into ``out`` ``(n_worlds, 2)`` (for example ``cpg.drive``)
        or into :attr:`drive`; returns the drive tensor."""
        h = self._handle()
        n = self.n_worlds
        t = self.sim._torch
        if isinstance(odor, t.Tensor) and odor.ndim == 3 and tuple(odor.shape[::2]) == (n, 4) and int(odor.shape[1]) <= self.odor_dim:
            raise ValueError(f"odor has {int(odor.shape[1])} dimensions, the navigator reads dimension {self.odor_dim}")
        n_dims = int(odor.shape[1]) if isinstance(odor, t.Tensor) and odor.ndim == 3 else self.odor_dim + 1
        self._checked("odor", odor, ((n, n_dims, 4),))
        self._checked("wind", wind, ((n, 2), (1, 2), (2,)))
        drive = self.drive if out is None else self._checked("out", out, ((n, 2),))
        rows = n if tuple(wind.shape) == (n, 2) else 1
        _native.check(_native.lib().nmf_navigator_update(h, odor.data_ptr(), n_dims, wind.data_ptr(), rows,
                                                         None if out is None else out.data_ptr(), self.sim._stream()))
        return drive

    def reset(self, mask=None) -> None:
        """The worlds of ``mask`` (``(n_worlds,)`` bool, numpy or torch; default all) start again: walking, empty filters, tick 0
        (their noise stream from its start), no encounters, the walk drive in :attr:`drive`; the others keep their state."""
        h = self._handle()
        m = reset_mask(mask, self.n_worlds, self.sim)
        _native.check(_native.lib().nmf_navigator_reset(h, None if m is None else m.data_ptr(), self.sim._stream()))


class _StabilizerParams(ctypes.Structure):
    """``nmf_stabilizer_params`` of include/nmf.h."""

    _fields_ = [("n_q", ctypes.c_int32), ("contacts", ctypes.c_int32), ("n_hidden", ctypes.c_int32), ("hidden", ctypes.c_int32 * 3),
                ("n_out", ctypes.c_int32), ("thr2", ctypes.c_float * 6), ("lo", ctypes.c_float * 8), ("hi", ctypes.c_float * 8)]


NECK_DOFS = ("c_thorax-c_head-roll", "c_thorax-c_head-pitch")
# The anatomy names a dof after its axis in the child segment's frame, x = yaw, y = pitch, z = roll (``RotationAxis.to_vector``: the
# legs' convention, z along the limb), and the head's frame is aligned with the thorax's at the neutral pose: forward kinematics
# shows the neck dof NAMED roll turning the head about the vertical axis and the one named yaw about the forward axis.  The outputs
# that cancel the thorax's world-frame roll and pitch (``HeadStabilizer.ideal_targets``) therefore belong on these two:
LEVELLING_NECK_DOFS = ("c_thorax-c_head-yaw", "c_thorax-c_head-pitch")


def _leg_contact_flags(torch, sensordata, thr2):
    """``(n, 6)`` float32 in torch: leg ``l`` touches (``found > 0``) with a squared net force above ``thr2[l]``."""
    sd = sensordata.reshape(-1, 6, 16)
    return ((sd[:, :, 0] > 0) & ((sd[:, :, 1:4] ** 2).sum(dim=2) > thr2)).to(torch.float32)


class HeadStabilizer(NativeHandle):
    """Head stabilization on the GPU (``nmf_stabilizer_*``): per world a small MLP from the leg joint angles and the leg contact
    flags to the neck's roll and pitch that cancel the thorax's rocking, so that the eyes (``EyeRenderer`` hangs its cameras on
    ``l_eye`` / ``r_eye``) see a steady horizon — the form of flygym 1.x's head-stabilization model.

    Build-defined and pinned by nothing (the reference ships no controllers; nothing is claimed about matching flygym 1.x, and
    nothing about how much steadier the gaze gets: ``examples/steady_the_gaze.py`` prints what it measures); the statement of the
    model is include/nmf.h (``nmf_stabilizer_update``), its specification in numpy tests/stabilizer_spec.py.  One :meth:`update`
    per control tick, from the batch's ``qpos`` and ``sensordata`` as they stand, in float32::

        x[k]       = (qpos[7 + input_dofs[k]] - input_mean[k]) * (1 / input_std[k])
        x[n_q + l] = leg l touches and |F_l|^2 > contact_force_thr[pair of l]^2 ? 1 : 0        (six flags, unless the threshold is None)
        h = x;  per layer (W, b):  a = b, then a[j] = fmaf(W[j, k], h[k], a[j]) for k ascending;  h = relu(a), the last layer: y = a
        out[j] = clip(y[j], limits);  ctrl[actuator of output_dofs[j]] = out[j]                  (with ``drive_actuators``)

    Args:
        sim: the batch; for a world with several flies ``sim.for_fly(fly_name)``.
        fly_name: the fly whose joints are read and whose neck is driven.
        layers: ``[(W, b), ...]`` float32, ``W`` ``(n_out_i, n_in_i)``: one to three hidden layers of 1..64 units and the output
            layer of 1..8 units; at most 256 inputs.
        input_dofs: joint dofs (``JointDOF`` or names) read as inputs; default the fly's leg dofs that have position actuators,
            in ``get_actuated_jointdofs_order("position")`` order (42 on ``make_model``'s flies).
        input_mean, input_std: per input dof (default 0 and 1): what :meth:`fit` returns.
        contact_force_thr: per leg pair front / middle / hind, in the contact sensors' force unit — flygym 1.x's values as
            remembered (its source is not at hand).  ``None`` drops the six flags.
        output_dofs: the joint dofs the outputs drive; default the neck dofs named roll and pitch (:data:`NECK_DOFS`).  In this
            anatomy's naming the dof that turns the head about the forward axis — what cancels a world-frame roll — is the one
            named yaw: a network trained on :meth:`ideal_targets` takes ``output_dofs=LEVELLING_NECK_DOFS`` (see there).
        limits: ``(lo, hi)``, scalars or one value per output.
        drive_actuators: write the outputs into the ``ctrl`` columns of the output dofs' position actuators.  ``False`` only
            fills ``out`` — usable on any skeleton, LEGS_ONLY included.

    ``output`` ``(n_worlds, n_out)`` float32 is the zero-copy view of the handle's own array.  :meth:`update` is one launch of
    stream-ordered device work on the simulation's stream and can be captured in a graph (with ``cpg.step``: the CPGs leave the
    neck's ``ctrl`` columns alone).  Close the stabilizer before its simulation.
    """

    _destroy_entry, _noun, _views = "nmf_stabilizer_destroy", "stabilizer", ("output",)

    def __init__(self, sim, fly_name: str, layers, *, input_dofs=None, input_mean=None, input_std=None,
                 contact_force_thr=(0.5, 1.0, 3.0), output_dofs=None, limits=(-np.pi / 2, np.pi / 2), drive_actuators: bool = True):
        sim = fly_batch(sim, fly_name, resolve=False)
        if fly_name not in sim.world.fly_lookup:
            raise ValueError(f"no fly named {fly_name!r} in this simulation ({', '.join(sim.world.fly_lookup)})")
        fly = sim.world.fly_lookup[fly_name]
        self.sim, self.fly_name, self.n_worlds = sim, fly_name, int(sim.n_worlds)
        self.layers = [(np.ascontiguousarray(W, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)) for W, b in layers]
        if not 2 <= len(self.layers) <= 4:
            raise ValueError(f"layers takes one to three hidden layers and the output layer, got {len(self.layers)} layers")
        all_dofs = [d.name for d in fly.get_jointdofs_order()]
        name_of = lambda d: d if isinstance(d, str) else d.name
        if input_dofs is None:
            input_dofs = [d for d in fly.get_actuated_jointdofs_order("position") if d.child.pos in LEGS]
        self.input_dofs = [name_of(d) for d in input_dofs]
        missing = [d for d in self.input_dofs if d not in all_dofs]
        if missing:
            raise ValueError(f"the fly has no joint dof {missing[0]!r}")
        self._dof = np.array([all_dofs.index(d) for d in self.input_dofs], dtype=np.int32)
        n_q = len(self.input_dofs)
        self.contacts = contact_force_thr is not None
        if self.contacts and len(contact_force_thr) != 3:
            raise ValueError(f"contact_force_thr takes three values (front, middle, hind legs) or None, got {contact_force_thr!r}")
        self.n_in, self.n_out = n_q + (6 if self.contacts else 0), int(self.layers[-1][0].shape[0]) if self.layers[-1][0].ndim == 2 else 0
        n_prev = self.n_in
        for i, (W, b) in enumerate(self.layers):
            if W.ndim != 2 or W.shape[1] != n_prev or b.shape != (W.shape[0],):
                raise ValueError(f"layer {i} must be (W (n, {n_prev}), b (n,)), got {tuple(W.shape)} and {tuple(b.shape)}")
            n_prev = int(W.shape[0])
        self._mean = np.zeros(n_q, dtype=np.float32) if input_mean is None else np.ascontiguousarray(input_mean, dtype=np.float32)
        std = np.ones(n_q, dtype=np.float32) if input_std is None else np.ascontiguousarray(input_std, dtype=np.float32)
        if self._mean.shape != (n_q,) or std.shape != (n_q,):
            raise ValueError(f"input_mean and input_std take one value per input dof ({n_q}), got {self._mean.shape} and {std.shape}")
        if not (std > 0).all():
            raise ValueError("input_std must be positive")
        self._inv_std = (1.0 / std.astype(np.float64)).astype(np.float32)       # divided in float64, rounded once
        bound = lambda v: np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float32), (self.n_out,)))
        if len(limits) != 2:
            raise ValueError(f"limits takes (lo, hi), got {limits!r}")
        self.lo, self.hi = bound(limits[0]), bound(limits[1])
        self._act = None
        if drive_actuators:
            self.output_dofs = [name_of(d) for d in (NECK_DOFS if output_dofs is None else output_dofs)]
            if len(self.output_dofs) != self.n_out:
                raise ValueError(f"the network has {self.n_out} outputs for {len(self.output_dofs)} output dofs")
            ids = {a["jointdof"].name: i for i, a in enumerate(fly.actuators) if a["kind"] == "position"}
            for d in self.output_dofs:
                if d not in ids:
                    raise ValueError(f"{d} has no position actuator to drive: on a skeleton with a neck (ALL_BIOLOGICAL, ALL_POSSIBLE) add "
                                     f"one with fly.add_actuators([JointDOF.from_name({d!r})], \"position\", kp=...) before the world is "
                                     "compiled, or pass drive_actuators=False to only fill `out`")
            self._act = np.array([ids[d] for d in self.output_dofs], dtype=np.int32)
        else:
            self.output_dofs = None if output_dofs is None else [name_of(d) for d in output_dofs]
        check_params(_StabilizerParams, "nmf_stabilizer_params_size", "controllers.py")
        thr = [float(contact_force_thr["fmh".index(leg[1])]) for leg in LEGS] if self.contacts else [0.0] * 6
        self.thr2 = np.array([t * t for t in thr], dtype=np.float32)
        widths = [int(W.shape[0]) for W, _ in self.layers[:-1]]
        pad = lambda a, n: [*a, *([0] * (n - len(a)))]
        self._params = _StabilizerParams(n_q, int(self.contacts), len(widths), (ctypes.c_int32 * 3)(*pad(widths[:3], 3)), self.n_out,
                                         (ctypes.c_float * 6)(*self.thr2.tolist()), (ctypes.c_float * 8)(*pad(self.lo.tolist()[:8], 8)),
                                         (ctypes.c_float * 8)(*pad(self.hi.tolist()[:8], 8)))
        self._weights = np.concatenate([a.ravel() for W, b in self.layers for a in (W, b)]).astype(np.float32)
        h = self._create("nmf_stabilizer_create", sim._batch_h, ctypes.byref(self._params), self._dof.ctypes.data, self._mean.ctypes.data,
                         self._inv_std.ctypes.data, self._weights.ctypes.data, None if self._act is None else self._act.ctypes.data)
        self.output = _field_view(sim, _native.lib().nmf_stabilizer_field_ptr, h, 0)

    def update(self, out=None):
        """One update of every world from the batch's ``qpos`` and ``sensordata`` as they stand.  One kernel launch, no allocation
        — capturable.  Writes the outputs into ``out`` (``(n_worlds, n_out)`` float32, contiguous, on the simulation's device) or
        into :attr:`output`, and with ``drive_actuators`` into ``ctrl``; returns the tensor it wrote."""
        h = self._handle()
        t = self.sim._torch
        if out is not None and (not isinstance(out, t.Tensor) or tuple(out.shape) != (self.n_worlds, self.n_out) or out.dtype != t.float32
                                or out.device != t.device(self.sim.device) or not out.is_contiguous()):
            got = f"{tuple(out.shape)} {out.dtype} on {out.device}" if isinstance(out, t.Tensor) else type(out).__name__
            raise ValueError(f"out must be a contiguous float32 tensor of shape {(self.n_worlds, self.n_out)} on {self.sim.device}, got {got}")
        _native.check(_native.lib().nmf_stabilizer_update(h, None if out is None else out.data_ptr(), self.sim._stream()))
        return self.output if out is None else out

    # ---- in torch, not bit-pinned: what the network is trained on
    @staticmethod
    def collect_inputs(sim, fly_name: str, input_dofs=None, contact_force_thr=(0.5, 1.0, 3.0)):
        """``(n_worlds, n_in)`` float32 on the simulation's device: the raw (not standardised) joint angles of ``input_dofs`` and,
        unless the threshold is None, the six contact flags — the inputs a :class:`HeadStabilizer` with these arguments reads,
        for :meth:`fit`."""
        sim = fly_batch(sim, fly_name, resolve=False)
        fly, t = sim.world.fly_lookup[fly_name], sim._torch
        if input_dofs is None:
            input_dofs = [d for d in fly.get_actuated_jointdofs_order("position") if d.child.pos in LEGS]
        all_dofs = [d.name for d in fly.get_jointdofs_order()]
        cols = t.as_tensor([7 + all_dofs.index(d if isinstance(d, str) else d.name) for d in input_dofs], device=sim.device)
        x = sim.field("qpos")[:, cols]
        if contact_force_thr is None:
            return x
        thr2 = t.as_tensor([float(contact_force_thr["fmh".index(leg[1])]) ** 2 for leg in LEGS], dtype=t.float32, device=sim.device)
        return t.cat([x, _leg_contact_flags(t, sim.field("sensordata"), thr2)], dim=1)

    @staticmethod
    def ideal_targets(root_quat):
        """``(..., 2)``: minus the thorax's roll and pitch (x-y-z Tait–Bryan angles of ``(..., 4)`` quaternions ``(w, x, y, z)``, a
        torch tensor on any device) — the neck angles that would keep the head level, the signal flygym 1.x trained against."""
        import torch

        w, x, y, z = root_quat.unbind(dim=-1)
        roll = torch.atan2(2 * (w * x + y * z), 1 - 2 * (x * x + y * y))
        pitch = torch.asin(torch.clamp(2 * (w * y - z * x), -1.0, 1.0))
        return torch.stack([-roll, -pitch], dim=-1)

    @staticmethod
    def fit(inputs, targets, hidden=(32, 32), *, epochs: int = 300, lr: float = 1e-2, n_flags: int = 6, seed: int = 0):
        """Train the MLP ``n_in -> hidden... -> n_out`` (ReLU; the default 32, 32 is flygym 1.x's three-layer network as remembered)
        on ``inputs`` ``(N, n_in)`` (the last ``n_flags`` columns are contact flags) against ``targets`` ``(N, n_out)``: full-batch
        Adam on the mean squared error, float32, on the CPU, deterministic for a given seed.  Only the joint columns are
        standardised.  Returns ``(layers, mean, std)`` for :class:`HeadStabilizer` — measured on some flies, used on others, as
        ``PathIntegrator.calibrate``."""
        import torch

        X = torch.as_tensor(inputs).detach().to("cpu", torch.float32)
        Y = torch.as_tensor(targets).detach().to("cpu", torch.float32)
        if X.ndim != 2 or Y.ndim != 2 or X.shape[0] != Y.shape[0] or X.shape[0] < 2 or not 0 <= int(n_flags) < X.shape[1]:
            raise ValueError(f"fit takes inputs (N, n_in) and targets (N, n_out) with N >= 2, got {tuple(X.shape)} and {tuple(Y.shape)}")
        n_q = X.shape[1] - int(n_flags)
        mean = X[:, :n_q].mean(dim=0)
        std = X[:, :n_q].std(dim=0).clamp_min(1e-6)
        Z = torch.cat([(X[:, :n_q] - mean) / std, X[:, n_q:]], dim=1)
        gen = torch.Generator().manual_seed(int(seed))
        sizes = [Z.shape[1], *[int(h) for h in hidden], Y.shape[1]]
        params = []
        for a, b in zip(sizes[:-1], sizes[1:]):
            W = (torch.rand((b, a), generator=gen) * 2 - 1) * (6.0 / (a + b)) ** 0.5
            params += [W.requires_grad_(), torch.zeros(b, requires_grad=True)]

        def forward(h):
            for i in range(0, len(params), 2):
                h = torch.nn.functional.linear(h, params[i], params[i + 1])
                if i + 2 < len(params):
                    h = torch.relu(h)
            return h

        opt = torch.optim.Adam(params, lr=float(lr))
        for _ in range(int(epochs)):
            opt.zero_grad()
            loss = ((forward(Z) - Y) ** 2).mean()
            loss.backward()
            opt.step()
        layers = [(params[i].detach().numpy().copy(), params[i + 1].detach().numpy().copy()) for i in range(0, len(params), 2)]
        return layers, mean.numpy().copy(), std.numpy().copy()
