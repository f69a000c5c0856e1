"""Batched, device-resident Pioneer-arm env (the RLlib ``VectorEnv`` shape with tensors).

Mirrors, for N envs at once, ``PioneerKinematicEnv`` of the reference
(pioneer/envs/pioneer/pioneer_knm_env.py:37-242): same constants, same
``reset_world`` override arguments, same step outputs; lists become torch
tensors that never leave the GPU.  All work happens in libpioneer_amd.so
(HIP); there is no Python or CPU compute path here.
"""
import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _lib
from .config import EngineConfig, PioneerKinematicConfig, SimulationConfig, fill_scene_body, to_c_config
from .model import LINK_NAMES
from .spaces import Box


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _rebuild_vector_env(ctor):
    return PioneerVectorEnv(**ctor)


class PioneerVectorEnv:
    """N independent Pioneer arms stepped by one HIP kernel launch.

    obs tensors are ``[N, 137]`` (``obs_layout="env_major"``) or ``[137, N]``
    (``"feature_major"``); actions ``[N, 6]`` / ``[6, N]``; rewards float32 ``[N]``;
    dones / truncated uint8 ``[N]``.
    """

    def __init__(self, num_envs: int, device=None, seed: int = 0, env_id_offset: int = 0,
                 pioneer_config: Optional[PioneerKinematicConfig] = None,
                 simulation_config: Optional[SimulationConfig] = None,
                 engine_config: Optional[EngineConfig] = None):
        self._h = None
        self._ctor = dict(num_envs=num_envs, device=device, seed=seed, env_id_offset=env_id_offset,
                          pioneer_config=pioneer_config, simulation_config=simulation_config,
                          engine_config=engine_config)
        self.lib = _lib.load_library()
        if not torch.cuda.is_available():
            raise RuntimeError("pioneer_amd needs a HIP device (torch.cuda.is_available() is False); "
                               "there is no CPU backend")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != "cuda":
            raise AssertionError(f"device must be a HIP device, got {self.device}")
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", dev_index)

        self.config = pioneer_config or PioneerKinematicConfig()
        self.simulation_config = simulation_config or SimulationConfig()
        self.engine_config = engine_config or EngineConfig()
        self.num_envs = int(num_envs)
        self.env_id_offset = int(env_id_offset)
        self._c_cfg = to_c_config(self.config, self.simulation_config, self.engine_config)

        k = _lib.PnrConstants()
        _lib.check(self.lib.pnr_get_constants(self._c_cfg, k))
        self.r_lo = np.array(k.r_lo[:], dtype=np.float32)    # pioneer_knm_env.py:56
        self.r_hi = np.array(k.r_hi[:], dtype=np.float32)
        self.v_max = np.array(k.v_max[:], dtype=np.float32)  # :57
        self.a_max = np.array(k.a_max[:], dtype=np.float32)  # :58
        self.dt = k.dt                                       # :60
        self.eps = k.eps                                     # :61
        self.dof = _lib.DOF
        self.obs_dim = _lib.OBS_DIM

        h = C.c_void_p()
        _lib.check(self.lib.pnr_create(self._c_cfg, self.num_envs, self.env_id_offset, dev_index,
                                       C.c_uint64(seed & (2**64 - 1)), C.byref(h)))
        self._h = h
        self._seed = seed
        self._body_on, self._body_params = False, None      # set_body: the moving sphere is enabled, under these params
        self._grip_on, self._grip_params = False, None      # set_body_grip: the grip is enabled, under these params
        self._body_queries = None                           # set_body_queries' arguments, once called (render: render_frames asks pnr_render_bodies)

        self.feature_major_obs = self.engine_config.obs_layout == "feature_major"
        self.feature_major_act = self.engine_config.action_layout == "feature_major"
        self.obs_shape = (self.obs_dim, self.num_envs) if self.feature_major_obs else (self.num_envs, self.obs_dim)
        self.action_shape = (self.dof, self.num_envs) if self.feature_major_act else (self.num_envs, self.dof)

        # spaces of ONE env, as the reference defines them (:72-74)
        self.action_space = Box(-self.a_max, self.a_max, dtype=np.float32)
        self.observation_space = Box(-np.inf, np.inf, shape=(self.obs_dim,), dtype=np.float32)
        self.reward_range = (-float("inf"), float("inf"))

    # -- plumbing -------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _check_handle(self):
        if self._h is None:
            raise RuntimeError("env is closed")

    def _chk(self, code):
        _lib.check(code, self._h)

    def _in(self, t, shape, dtype, name):
        if not isinstance(t, torch.Tensor):
            t = torch.as_tensor(np.asarray(t), dtype=dtype)
        if t.device != self.device or t.dtype != dtype:
            t = t.to(device=self.device, dtype=dtype)
        if tuple(t.shape) != tuple(shape):
            raise AssertionError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
        return t.contiguous()

    def _new(self, shape, dtype=torch.float32):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def _out(self, out, key, shape, dtype=torch.float32, check=True):
        """The caller's output tensor (``out`` itself, or ``out[key]`` of a dict of them) or, without one, a new tensor.
        ``check``: the caller's must have this shape and be written in place; else (vector_step, rollout) it is taken as given."""
        t = out.get(key) if hasattr(out, "get") else out
        if t is None:
            return self._new(shape, dtype)
        if not check:
            return t
        res = self._in(t, shape, dtype, key)
        assert res.data_ptr() == t.data_ptr(), f"{key} is written in place: it must already be a contiguous {dtype} device tensor"
        return res

    def _joints(self, joint_state):
        """A query's optional ``joint_state`` ``[N, 12]`` (q | qd) as a float32 device tensor; None = the handle's own joints."""
        return None if joint_state is None else self._in(joint_state, (self.num_envs, 12), torch.float32, "joint_state")

    def _asked(self, out, specs, nothing):
        """The outputs asked for ((key, wanted, shape, dtype) in ``specs``), from ``out`` or new; none: AssertionError(``nothing``)."""
        res = {key: self._out(out or {}, key, shape, dtype) for key, want, shape, dtype in specs if want}
        if not res:
            raise AssertionError(nothing)
        return res

    # -- gym-ish surface ----------------------------------------------------------------
    def seed(self, seed=None):
        """pioneer_knm_env.py:107-109 (takes effect at the next reset)."""
        self._check_handle()
        if seed is None:
            seed = int(np.random.SeedSequence().entropy & (2**63 - 1))
        self._seed = int(seed)
        self._chk(self.lib.pnr_seed(self._h, C.c_uint64(self._seed & (2**64 - 1))))
        return [self._seed]

    def reset(self, mask=None, joint_positions=None, target_positions=None, out=None):
        """BulletEnv.reset + reset_world (bullet_env.py:187-190, pioneer_knm_env.py:76-105).

        ``mask`` selects envs (uint8/bool ``[N]``; None = all); ``joint_positions``
        ``[N,6]`` / ``target_positions`` ``[N,3]`` override the random draws as the
        reference's arguments do.  Returns the obs batch (rows of unselected envs
        are only meaningful if ``out`` already held them).
        """
        self._check_handle()
        n = self.num_envs
        m = None if mask is None else self._in(torch.as_tensor(mask).to(torch.uint8), (n,), torch.uint8, "mask")
        jp = None if joint_positions is None else self._in(joint_positions, (n, 6), torch.float32, "joint_positions")
        tp = None if target_positions is None else self._in(target_positions, (n, 3), torch.float32, "target_positions")
        obs = self._out(out, "out", self.obs_shape)
        if out is None and m is not None:
            self._chk(self.lib.pnr_observe(self._h, _ptr(obs), self._stream()))
        self._chk(self.lib.pnr_reset(self._h, _ptr(m), _ptr(jp), _ptr(tp), _ptr(obs), self._stream()))
        return obs

    def vector_reset(self):
        return self.reset()

    def reset_at(self, index: int):
        """RLlib VectorEnv.reset_at: reset one env, return its obs row (env-major order)."""
        mask = torch.zeros(self.num_envs, dtype=torch.uint8, device=self.device)
        mask[index] = 1
        obs = self.reset(mask=mask)
        return obs[:, index] if self.feature_major_obs else obs[index]

    def vector_step(self, actions, out=None, want_info=False):
        """BulletEnv.step for every env (bullet_env.py:192-197).

        Returns ``(obs, rewards, dones, truncated)`` (+ ``info [N,4]`` =
        r_pot, r_step, r_done, dist when ``want_info``).  ``out`` may carry
        preallocated ``obs/reward/done/truncated/info`` tensors.
        """
        self._check_handle()
        n = self.num_envs
        act = self._in(actions, self.action_shape, torch.float32, "actions")
        out = out or {}
        obs = self._out(out, "obs", self.obs_shape, check=False)
        rew = self._out(out, "reward", (n,), check=False)
        done = self._out(out, "done", (n,), torch.uint8, check=False)
        trunc = self._out(out, "truncated", (n,), torch.uint8, check=False)
        info = self._out(out, "info", (n, _lib.INFO_DIM), check=False) if want_info else None
        self._chk(self.lib.pnr_step(self._h, _ptr(act), _ptr(obs), _ptr(rew), _ptr(done), _ptr(trunc),
                                    _ptr(info), self._stream()))
        if want_info:
            return obs, rew, done, trunc, info
        return obs, rew, done, trunc

    def rollout(self, actions, out=None):
        """T open-loop steps in one launch; ``actions`` is ``[T, *action_shape]``."""
        self._check_handle()
        n = self.num_envs
        T = int(actions.shape[0])
        act = self._in(actions, (T,) + tuple(self.action_shape), torch.float32, "actions")
        out = out or {}
        obs = self._out(out, "obs", (T,) + tuple(self.obs_shape), check=False)
        rew = self._out(out, "reward", (T, n), check=False)
        done = self._out(out, "done", (T, n), torch.uint8, check=False)
        trunc = self._out(out, "truncated", (T, n), torch.uint8, check=False)
        self._chk(self.lib.pnr_rollout(self._h, T, _ptr(act), _ptr(obs), _ptr(rew), _ptr(done), _ptr(trunc),
                                       self._stream()))
        return obs, rew, done, trunc

    def _wrench_specs(self, specs):
        """``world_step``'s ``(link, frame)`` pairs as a pnr_link_wrench_spec array: link an index or a ``LINK_NAMES`` name, frame
        ``"link"`` / ``"world"``.  The count and the index range are the engine's to refuse."""
        frames = {"link": _lib.FRAME_LINK, "world": _lib.FRAME_WORLD}
        arr = (_lib.PnrLinkWrenchSpec * max(len(specs), 1))()
        for j, (link, frame) in enumerate(specs):
            if isinstance(link, str):
                if link not in LINK_NAMES:
                    raise AssertionError(f"world_step: no link named {link!r}")
                link = LINK_NAMES.index(link)
            if frame not in frames:
                raise AssertionError(f"world_step: frame must be 'link' or 'world', got {frame!r}")
            arr[j].link, arr[j].frame = int(link), frames[frame]
        return arr

    def world_step(self, joint_state=None, joint_torques=None, link_wrenches=None, hold_substeps=None, motor_targets=None,
                   motor_joints=None):
        """World.step() alone (bullet_scene.py:273-275; pnr_world_step): the simulator's sub-steps and nothing else.  Dynamics mode:
        ``joint_state`` is None (the handle's q, qd move); kinematic mode: the caller's float32 [N, 12] device buffer (q | qd).
        ``joint_torques`` (dynamics mode; float32 ``[N, 6]`` on the env's device, only read): PyBullet's TORQUE_CONTROL
        (pnr_world_step_torques) — added to each joint's torque in every sub-step of this call only, next to the joints' motors as
        ``set_joint_motor`` left them (zero gains first for pure torque control).
        ``link_wrenches`` (dynamics mode) = ``(specs, tensor)``: PyBullet's applyExternalForce / applyExternalTorque
        (pnr_world_step_wrenches), in the same launch as ``joint_torques`` when both are given.  ``specs``: up to
        ``_lib.MAX_LINK_WRENCHES`` pairs ``(link, frame)``, the same for every env — ``link`` an index 0..10 or a ``LINK_NAMES``
        name, ``frame`` ``"link"`` or ``"world"``; ``tensor``: float32 ``[N, K, 9]`` on the env's device, only read, per record
        force[3] | position[3] | torque[3] in that frame (``"world"``: a world point, taken on the link at the call's first pose;
        ``"link"``: a point of the link's frame).  ``hold_substeps``: the records act in that many of the call's first sub-steps
        (None, <= 0 or >= frame_skip: all of them; 1: Bullet's literal clearing after one stepSimulation).
        ``motor_targets`` (dynamics mode; float32 ``[N, 12]`` on the env's device, only read): PyBullet's
        setJointMotorControlArray per env (pnr_world_step_targets) — position[6] | velocity[6], each env's own targetPosition /
        targetVelocity for the joints of ``motor_joints`` (an iterable of joint indices 0..5; None: all six), for this call only;
        law, gains, force cap and maxVelocity of each joint stay as ``set_joint_motor`` left them (a joint nobody commanded: the
        EngineConfig's law, the targets standing in for the env's command state).  The other joints' entries are ignored (NaN is
        fine); the position entry of a joint on a velocity law must be finite.  Combines with ``joint_torques`` (same launch), not
        with ``joint_state`` or ``link_wrenches``.  With a moving sphere enabled (``set_body``) the same calls move it too;
        ``link_wrenches`` and a constraint motor next to it are the engine's to refuse.  Never synchronises."""
        self._check_handle()
        if motor_targets is not None:
            if joint_state is not None:
                raise AssertionError("world_step: motor_targets drive the handle's simulated joints; joint_state must be None")
            if link_wrenches is not None:
                raise AssertionError("world_step: per-env motor_targets together with link_wrenches is not built "
                                     "(pnr_world_step_targets takes joint_torques only)")
            if hold_substeps is not None:
                raise AssertionError("world_step: hold_substeps belongs to link_wrenches")
            joints = range(6) if motor_joints is None else [int(j) for j in motor_joints]
            if any(j < 0 or j >= 6 for j in joints):
                raise AssertionError(f"world_step: motor_joints must be joint indices 0..5, got {list(joints)}")
            mask = 0
            for j in joints:
                mask |= 1 << j
            tg = self._in(motor_targets, (self.num_envs, 12), torch.float32, "motor_targets")
            tq = None if joint_torques is None else self._in(joint_torques, (self.num_envs, 6), torch.float32, "joint_torques")
            self._chk(self.lib.pnr_world_step_targets(self._h, mask, _ptr(tg), _ptr(tq), self._stream()))
            return
        if motor_joints is not None:
            raise AssertionError("world_step: motor_joints belongs to motor_targets")
        if link_wrenches is not None:
            if joint_state is not None:
                raise AssertionError("world_step: link_wrenches act on the handle's simulated joints; joint_state must be None")
            specs, tensor = link_wrenches
            specs = list(specs)
            arr = self._wrench_specs(specs)
            wr = self._in(tensor, (self.num_envs, len(specs), _lib.WRENCH_DIM), torch.float32, "link_wrenches")
            tq = None if joint_torques is None else self._in(joint_torques, (self.num_envs, 6), torch.float32, "joint_torques")
            self._chk(self.lib.pnr_world_step_wrenches(self._h, arr, len(specs), _ptr(wr), _ptr(tq),
                                                       0 if hold_substeps is None else int(hold_substeps), self._stream()))
            return
        if hold_substeps is not None:
            raise AssertionError("world_step: hold_substeps belongs to link_wrenches")
        if joint_torques is not None:
            if joint_state is not None:
                raise AssertionError("world_step: joint_torques act on the handle's simulated joints; joint_state must be None")
            tq = self._in(joint_torques, (self.num_envs, 6), torch.float32, "joint_torques")
            self._chk(self.lib.pnr_world_step_torques(self._h, _ptr(tq), self._stream()))
            return
        js = None if joint_state is None else self._out(joint_state, "joint_state", (self.num_envs, 12))
        self._chk(self.lib.pnr_world_step(self._h, _ptr(js), self._stream()))

    # -- the moving sphere ----------------------------------------------------------------
    def set_body(self, params=None, *, mass=None, radius=None, position=None, velocity=None, mask=None):
        """One moving sphere per env that ``world_step`` integrates with the arm (pnr_set_body_params + pnr_set_body_state;
        createMultiBody(baseMass > 0), bullet_scene.py:230-246): a point mass with a radius — position and linear velocity, no
        orientation, no spin; rolling is not modelled.  It collides with the arm's contact samples (the pointer's; all 23 with
        ``link_contacts``) and with everything static; include/pioneer_amd.h states the law.  ``params``: a dict of
        ``contact_kp, contact_kd`` (default: the EngineConfig's), ``friction`` (0.5), ``slip_eps`` (0.05), ``linear_damping`` (0);
        ``False`` disables the sphere (its state is kept).  ``mass`` / ``radius``: a number or ``[N]``; ``position`` /
        ``velocity``: ``[3]`` or ``[N, 3]``; each left out keeps what the envs hold (all zero before the first call: mass 0 = no
        sphere in that env, which takes and gives no force).  ``mask`` (``[N]`` bool / uint8): only these envs' words are written.
        Stability of the explicit penalty spring needs ``contact_kd * timestep < mass`` and ``contact_kp * timestep**2 < mass``
        (mass > 0.21 with the defaults).  ``vector_step`` / ``rollout`` / ``reset`` neither move nor see the sphere;
        ``render_frames`` / ``ray_test`` / ``contacts`` see it once ``set_body_queries`` says so.  The first call allocates and
        waits for the buffer's zero fill."""
        self._check_handle()
        if params is False:
            self._chk(self.lib.pnr_set_body_params(self._h, None))
            self._body_on = False
            return
        if params is None and self._body_on:                   # a later call without params keeps them
            params = self._body_params
        p = _lib.PnrBodyParams()
        _lib.check(self.lib.pnr_body_params_default(p))
        for k, v in (params or {}).items():
            if k not in ("contact_kp", "contact_kd", "friction", "slip_eps", "linear_damping"):
                raise AssertionError(f"set_body: unknown parameter {k!r}")
            setattr(p, k, float(v))
        self._chk(self.lib.pnr_set_body_params(self._h, p))
        self._body_on, self._body_params = True, dict(params or {})
        given = dict(mass=mass, radius=radius, position=position, velocity=velocity)
        if all(v is None for v in given.values()):
            return
        n = self.num_envs
        w = self.body_state().T.contiguous()                                      # [8, N]
        rows = dict(position=slice(0, 3), velocity=slice(3, 6), mass=slice(6, 7), radius=slice(7, 8))
        for k, v in given.items():
            if v is None:
                continue
            t = torch.as_tensor(np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v), dtype=torch.float32).to(self.device)
            width = rows[k].stop - rows[k].start
            t = t.reshape(-1, width) if width == 3 else t.reshape(-1, 1)
            if t.shape[0] not in (1, n):
                raise AssertionError(f"set_body: {k} must be one value or one per env")
            w[rows[k]] = t.expand(n, width).T
        self.set_body_state(w.T, mask=mask)

    def set_body_queries(self, render=False, rays=False, contacts=False, rgba=None):
        """Which batched scene queries see the moving sphere (pnr_set_body_queries; all off after construction, which is every
        query as it always was): ``render`` draws it in ``render_frames`` (label ``_lib.SEG_MOVING_BODY`` = 21, colour ``rgba``,
        initially the obstacle material's grey; None keeps the current colour), ``rays`` lets ``ray_test`` hit it with
        ``hit_bodies`` (label 21, after the caller's bodies on a tie), ``contacts`` makes ``contacts`` report it as body
        ``_lib.MAX_SCENE`` (8) with the step's arm-sphere law on the relative velocity.  Each query reads the spheres' state of the
        moment it runs, per env: mass > 0 = a sphere, its own centre, velocity and radius.  A host-side switch: no launch.  Needs a
        first ``set_body`` (the buffer)."""
        self._check_handle()
        bits = (_lib.BODY_IN_RENDER if render else 0) | (_lib.BODY_IN_RAYS if rays else 0) | (_lib.BODY_IN_CONTACTS if contacts else 0)
        col = None if rgba is None else (C.c_float * 4)(*(float(v) for v in rgba))
        self._chk(self.lib.pnr_set_body_queries(self._h, bits, col))
        rgba = rgba if rgba is not None or self._body_queries is None else self._body_queries["rgba"]
        self._body_queries = dict(render=bool(render), rays=bool(rays), contacts=bool(contacts), rgba=rgba)

    def body_state(self):
        """The spheres' state, float32 ``[N, 8]`` on the device: position[3] | velocity[3] | mass | radius (pnr_get_body_state; the
        base-item branch of Item.pose / Item.velocity, bullet_scene.py:53-68)."""
        self._check_handle()
        w = self._new((_lib.BODY_STATE_WORDS, self.num_envs))
        self._chk(self.lib.pnr_get_body_state(self._h, _ptr(w), self._stream()))
        return w.T

    def set_body_state(self, words, mask=None):
        """``words`` ``[N, 8]`` (as ``body_state``) into the envs of ``mask`` (``[N]`` bool / uint8 on any device; None: all): the
        device-side reset of a sphere (pnr_set_body_state; resetBasePositionAndOrientation, bullet_scene.py:70-73)."""
        self._check_handle()
        n = self.num_envs
        w = self._in(words, (n, _lib.BODY_STATE_WORDS), torch.float32, "words").T.contiguous()
        m = None if mask is None else self._in(torch.as_tensor(mask).to(torch.uint8), (n,), torch.uint8, "mask")
        self._chk(self.lib.pnr_set_body_state(self._h, _ptr(w), _ptr(m), self._stream()))
        torch.cuda.current_stream(self.device).synchronize()  # `w` and `m` are temporaries

    # -- the grip on the moving sphere ----------------------------------------------------
    _GRIP_FIELDS = ("anchor", "direction", "grip_kp", "grip_kd")

    def _grip_params_struct(self, params):
        p = _lib.PnrBodyGripParams()
        _lib.check(self.lib.pnr_body_grip_params_default(p))
        for k, v in (params or {}).items():
            if k not in self._GRIP_FIELDS:
                raise AssertionError(f"set_body_grip: unknown parameter {k!r}")
            if k in ("anchor", "direction"):
                v = tuple(float(c) for c in v)
                assert len(v) == 3, f"set_body_grip: {k} is a 3-vector"
                setattr(p, k, (C.c_float * 3)(*v))
            else:
                setattr(p, k, float(v))
        return p

    def set_body_grip(self, params=None, *, max_force=None, mask=None):
        """The grip: each env's moving sphere held at a point of link ``robot:pointer`` by a soft point-to-point constraint with a
        force cap (pnr_set_body_grip_params + pnr_set_body_grip; PyBullet's createConstraint(JOINT_POINT2POINT) /
        changeConstraint(maxForce) / removeConstraint; include/pioneer_amd.h states the law).  ``params``: a dict of ``anchor``
        (0, 0, 0), ``direction`` (the unit vector along the tip offset: the held sphere sits tangent to the pointer's sample
        sphere; (0, 0, 0): the anchor is a plain point of the link), ``grip_kp``, ``grip_kd`` (default: the sphere's contact
        gains); ``False`` disables the grip (the buffer is kept and ``world_step`` runs the kernels without it).  ``max_force``: a
        number or ``[N]``, each env's force cap; <= 0 releases.  ``mask`` (``[N]`` bool / uint8 on any device): only these envs'
        words are written — "grip the envs that just came within reach".  A gripped env's sphere takes no contact from the arm;
        the static world still holds it.  Needs ``set_body`` first; the first call allocates and waits for the buffer's zero
        fill.  ``contacts()`` does not know the grip and keeps reporting the overlap of a held sphere."""
        self._check_handle()
        if params is False:
            self._chk(self.lib.pnr_set_body_grip_params(self._h, None))
            self._grip_on = False
            return
        if params is None and self._grip_on:                   # a later call without params keeps them
            params = self._grip_params
        p = self._grip_params_struct(params)
        self._chk(self.lib.pnr_set_body_grip_params(self._h, p))
        self._grip_on, self._grip_params = True, dict(params or {})
        if max_force is None:
            return
        n = self.num_envs
        f = torch.as_tensor(np.asarray(max_force.detach().cpu() if isinstance(max_force, torch.Tensor) else max_force), dtype=torch.float32)
        if f.numel() not in (1, n):
            raise AssertionError("set_body_grip: max_force must be one value or one per env")
        f = f.reshape(-1).expand(n).contiguous().to(self.device)
        m = None if mask is None else self._in(torch.as_tensor(mask).to(torch.uint8), (n,), torch.uint8, "mask")
        self._chk(self.lib.pnr_set_body_grip(self._h, _ptr(f), _ptr(m), self._stream()))
        torch.cuda.current_stream(self.device).synchronize()  # `f` and `m` are temporaries

    def body_grip(self):
        """The grips' state, float32 ``[N, 4]`` on the device: max_force | the world-frame force on the sphere in the last sub-step
        of the last ``world_step`` [3] (pnr_get_body_grip; getConstraintState).  Zero force for an env that was not gripped."""
        self._check_handle()
        w = self._new((_lib.BODY_GRIP_WORDS, self.num_envs))
        self._chk(self.lib.pnr_get_body_grip(self._h, _ptr(w), self._stream()))
        return w.T

    def grip_anchor(self):
        """The world position ``[N, 3]`` (float32, on the device) of each env's anchor point, where the grip holds the sphere's
        centre: the pointer link's pose (``link_states``) applied to ``anchor + (radius + pointer_radius) * direction`` with the
        env's radius (``body_state``) and the grip's params (the defaults before ``set_body_grip``).  Plain torch: it lets a caller
        write ``mask = (body_state()[:, :3] - grip_anchor()).norm(dim=1) < reach`` without restating the geometry."""
        self._check_handle()
        p = self._grip_params_struct(self._grip_params if self._grip_on else None)
        anchor = torch.tensor(p.anchor[:], dtype=torch.float32, device=self.device)
        direction = torch.tensor(p.direction[:], dtype=torch.float32, device=self.device)
        if float(direction.norm()) > 0:
            direction = direction / direction.norm()
        link = self.link_states()[:, _lib.NUM_LINKS - 1]                              # robot:pointer
        pos, (x, y, z, w) = link[:, 0:3], link[:, 3:7].unbind(dim=1)
        R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                         2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                         2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
        reach = self.body_state()[:, 7:8] + float(self.engine_config.pointer_radius)
        return pos + torch.einsum("nij,nj->ni", R, anchor[None, :] + reach * direction[None, :])

    def inverse_dynamics(self, joint_accel=None, joint_state=None, gravity=True, joint_losses=False, out=None):
        """calculateInverseDynamics of every env, one launch (pnr_inverse_dynamics): float32 ``[N, 6]`` joint torques
        tau = M(q) q̈ + C(q, q̇) q̇ + G(q) on the model the dynamics mode steps.  ``joint_accel``: ``[N, 6]`` q̈ (None = 0: the bias
        forces).  ``joint_state``: as ``link_states`` (``[N, 12]`` = q | q̇; None = the handle's own joints).  ``gravity=False``
        leaves G(q) out; ``joint_losses=True`` adds the engine's joint damping and friction at q̇, so that
        ``world_step(joint_torques=tau)`` realises q̈ away from contacts and limits.  Dynamics mode uses the handle's per-env link
        scales (and friction / damping); kinematic mode the nominal model.  Never synchronises."""
        self._check_handle()
        n = self.num_envs
        js = self._joints(joint_state)
        acc = None if joint_accel is None else self._in(joint_accel, (n, 6), torch.float32, "joint_accel")
        flags = (0 if gravity else _lib.INVDYN_NO_GRAVITY) | (_lib.INVDYN_JOINT_LOSSES if joint_losses else 0)
        res = self._out(out, "out", (n, 6))
        self._chk(self.lib.pnr_inverse_dynamics(self._h, _ptr(js), _ptr(acc), flags, _ptr(res), self._stream()))
        return res

    def mass_matrix(self, joint_state=None, out=None):
        """calculateMassMatrix of every env, one launch (pnr_mass_matrix): float32 ``[N, 6, 6]``, the symmetric joint-space inertia
        M(q) of the same model (``out[:, i, j] == out[:, j, i]`` bit for bit).  ``joint_state``: as ``inverse_dynamics`` (only q is
        read).  Never synchronises."""
        self._check_handle()
        n = self.num_envs
        js = self._joints(joint_state)
        res = self._out(out, "out", (n, 6, 6))
        self._chk(self.lib.pnr_mass_matrix(self._h, _ptr(js), _ptr(res), self._stream()))
        return res

    def joint_states(self, joint_state=None, joint_torques=None, link_wrenches=None, reaction=True, out=None):
        """getJointState of every env, one launch (pnr_get_joint_states; dynamics mode): what the first sub-step of
        ``world_step`` with the same ``joint_torques`` / ``link_wrenches`` would evaluate, looked at and not taken.  Returns a dict of
        device tensors: ``joints`` float32 ``[N, 6, 4]`` = q, q̇, q̈, τ_motor per joint (q̈ before the integrator and its joint-limit
        clamp; τ_motor the joint's own motor after its cap, without the caller's torques, damping or friction) and, with
        ``reaction``, ``reaction`` float32 ``[N, 6, 6]`` = (Fx, Fy, Fz, Mx, My, Mz) per joint: the wrench the parent exerts on the
        joint's child body, at the child link's origin in the child link's frame; its moment along the joint axis is the joint's
        total torque.  ``joint_state``: as ``link_states`` (None = the simulated q, q̇).  ``joint_torques`` and ``link_wrenches =
        (specs, tensor)``: as ``world_step`` (a world-frame record's point is taken at the current pose).  ``out`` may carry
        preallocated ``joints`` / ``reaction`` tensors, written in place.  Never synchronises."""
        self._check_handle()
        n = self.num_envs
        js = self._joints(joint_state)
        tq = None if joint_torques is None else self._in(joint_torques, (n, 6), torch.float32, "joint_torques")
        arr, wr, k = None, None, 0
        if link_wrenches is not None:
            specs, tensor = link_wrenches
            specs = list(specs)
            arr, k = self._wrench_specs(specs), len(specs)
            wr = self._in(tensor, (n, k, _lib.WRENCH_DIM), torch.float32, "link_wrenches")
        res = self._asked(out, (("joints", True, (n, _lib.DOF, _lib.JOINT_STATE_DIM), torch.float32),
                                ("reaction", reaction, (n, _lib.DOF, _lib.REACTION_DIM), torch.float32)), "")
        self._chk(self.lib.pnr_get_joint_states(self._h, _ptr(js), _ptr(tq), arr, k, _ptr(wr), _ptr(res["joints"]),
                                                _ptr(res.get("reaction")), self._stream()))
        return res

    def set_joint_motor(self, joint, control_mode, target_position=float("nan"), target_velocity=float("nan"), position_gain=float("nan"),
                        velocity_gain=float("nan"), max_force=float("nan"), max_velocity=float("nan")):
        """Joint.control_position / control_velocity (bullet_scene.py:123-155; pnr_set_joint_motor) for ``joint`` of every env.
        ``control_mode``: ``_lib.CONTROL_POSITION`` / ``CONTROL_VELOCITY`` (the PD torque law; NaN = the EngineConfig's value) or
        ``_lib.CONTROL_POSITION_CONSTRAINT`` / ``CONTROL_VELOCITY_CONSTRAINT`` (Bullet's constraint motor; NaN = Bullet's value,
        ``max_force`` 0 = no motor).  Honoured by ``world_step``."""
        self._check_handle()
        self._chk(self.lib.pnr_set_joint_motor(self._h, int(joint), int(control_mode), float(target_position), float(target_velocity),
                                               float(position_gain), float(velocity_gain), float(max_force), float(max_velocity)))

    def link_states(self, joint_state=None, out=None):
        """Item.pose() / Item.velocity() of every link of every env (bullet_scene.py:53-67; pnr_get_link_states), one launch:
        float32 ``[N, 11, 13]`` on the env's device, link k = ``LINK_NAMES[k]``; per link position[3], quaternion (x, y, z, w)
        with w >= 0 [4], linear velocity of the link frame origin [3], angular velocity [3], all in the world frame.
        ``joint_state`` (optional, ``[N, 12]`` = q | qd, only read): the kinematics of those joints; None = the handle's own
        (dynamics mode: the simulated q, qd; kinematic mode: the env's r, v)."""
        self._check_handle()
        n = self.num_envs
        js = self._joints(joint_state)
        res = self._out(out, "out", (n, _lib.NUM_LINKS, _lib.LINK_STATE_DIM))
        self._chk(self.lib.pnr_get_link_states(self._h, _ptr(js), _ptr(res), self._stream()))
        return res

    def jacobian(self, link=10, local_point=None, joint_state=None, out=None):
        """calculateJacobian of link ``link`` (0..10, ``LINK_NAMES`` order; default robot:pointer) of every env, one launch
        (pnr_get_jacobian): float32 ``[N, 6, 6]`` on the env's device.  Rows 0-2: world linear velocity of ``local_point`` (a
        point in the link's frame, default its origin) per unit velocity of joint j (column j); rows 3-5: the link's world
        angular velocity per unit joint velocity.  Columns of joints beyond the link are exactly 0.  ``joint_state``: as
        ``link_states`` (``[N, 12]`` = q | qd, only q is read; None = the handle's own joints).  Never synchronises."""
        self._check_handle()
        n = self.num_envs
        js = self._joints(joint_state)
        lp = None if local_point is None else (C.c_double * 3)(*(float(v) for v in local_point))
        res = self._out(out, "out", (n, 6, 6))
        self._chk(self.lib.pnr_get_jacobian(self._h, _ptr(js), int(link), lp, _ptr(res), self._stream()))
        return res

    def solve_ik(self, target=None, q_init=None, link=10, local_point=None, max_iterations=32, damping=1.0, max_step=0.5,
                 tolerance=1e-3, out=None):
        """calculateInverseKinematics (position only) for every env, one launch (pnr_solve_ik): joint angles inside the limits
        that put ``local_point`` of ``link`` on ``target`` (``[N, 3]`` world positions; None = each env's own target), by the
        damped-least-squares iteration of include/pioneer_amd.h from ``q_init`` (``[N, 6]``; None = the rest pose q = 0, from
        which every target of the reachable inner box converges; random starts end in local minima at joint limits).
        Returns ``(q [N, 6] float32, residual [N] float32, iterations [N] int32)``: residual is the distance left,
        iterations == max_iterations where the tolerance was never met (the target is out of reach, or the start was bad).
        ``out`` may carry preallocated ``q`` / ``residual`` / ``iterations`` tensors, written in place.  Never synchronises."""
        self._check_handle()
        n = self.num_envs
        p = _lib.PnrIkParams()
        self._chk(self.lib.pnr_ik_params_default(p))
        p.link, p.max_iterations = int(link), int(max_iterations)
        if local_point is not None:
            for k in range(3):
                p.local_point[k] = float(local_point[k])
        p.damping, p.max_step, p.tolerance = float(damping), float(max_step), float(tolerance)
        tgt = None if target is None else self._in(target, (n, 3), torch.float32, "target")
        qi = None if q_init is None else self._in(q_init, (n, 6), torch.float32, "q_init")
        out = out or {}
        q = self._out(out, "q", (n, 6))
        res = self._out(out, "residual", (n,))
        its = self._out(out, "iterations", (n,), torch.int32)
        self._chk(self.lib.pnr_solve_ik(self._h, p, _ptr(tgt), _ptr(qi), _ptr(q), _ptr(res), _ptr(its), self._stream()))
        return q, res, its

    def solve_ik_pose(self, target_orientation, target=None, q_init=None, link=10, local_point=None, align_axis=None,
                      max_iterations=32, damping=0.03, error_damping=0.01, orientation_weight=10.0, max_step=0.5, tolerance=1e-3,
                      angle_tolerance=1e-3, out=None):
        """calculateInverseKinematics with a targetOrientation for every env, one launch (pnr_solve_ik_pose): joint angles inside
        the limits that put ``local_point`` of ``link`` on ``target`` (``[N, 3]``; None = each env's own target) and turn the
        link to ``target_orientation`` (``[N, 4]`` quaternions x, y, z, w; normalised by the kernel).  ``align_axis`` None asks
        for the full orientation; a 3-vector in the link's frame asks only for that axis to point along the target's (the roll
        about it stays free).  The error-damped least-squares iteration of include/pioneer_amd.h from ``q_init`` (``[N, 6]``;
        None = the rest pose: pointing tasks converge from it, 88 % of full poses do; starts near a solution all converge).
        Returns ``(q [N, 6] float32, residual [N] float32, angle [N] float32 rad, iterations [N] int32)``; iterations ==
        max_iterations where the tolerances were never met.  ``out`` may carry preallocated ``q`` / ``residual`` / ``angle`` /
        ``iterations`` tensors, written in place.  Never synchronises."""
        self._check_handle()
        n = self.num_envs
        p = _lib.PnrIkPoseParams()
        self._chk(self.lib.pnr_ik_pose_params_default(p))
        p.link, p.max_iterations = int(link), int(max_iterations)
        if local_point is not None:
            for k in range(3):
                p.local_point[k] = float(local_point[k])
        if align_axis is not None:
            p.mode = _lib.IK_ORIENT_AXIS
            for k in range(3):
                p.local_axis[k] = float(align_axis[k])
        p.damping, p.error_damping, p.orientation_weight = float(damping), float(error_damping), float(orientation_weight)
        p.max_step, p.tolerance, p.angle_tolerance = float(max_step), float(tolerance), float(angle_tolerance)
        quat = self._in(target_orientation, (n, 4), torch.float32, "target_orientation")
        tgt = None if target is None else self._in(target, (n, 3), torch.float32, "target")
        qi = None if q_init is None else self._in(q_init, (n, 6), torch.float32, "q_init")
        out = out or {}
        q = self._out(out, "q", (n, 6))
        res = self._out(out, "residual", (n,))
        ang = self._out(out, "angle", (n,))
        its = self._out(out, "iterations", (n,), torch.int32)
        self._chk(self.lib.pnr_solve_ik_pose(self._h, p, _ptr(tgt), _ptr(quat), _ptr(qi), _ptr(q), _ptr(res), _ptr(ang), _ptr(its),
                                             self._stream()))
        return q, res, ang, its

    def solve_ik_multi(self, target_orientation=None, target=None, starts=8, q_init=None, q_ref=None, policy="best", align_axis=None,
                       link=10, local_point=None, max_iterations=32, damping=None, error_damping=None, orientation_weight=10.0,
                       max_step=0.5, tolerance=1e-3, angle_tolerance=1e-3, seed=0, return_all=False, out=None):
        """Multi-start inverse kinematics for every env, one launch (pnr_solve_ik_multi): S descents per env, and of the solutions
        found the one nearest to ``q_ref``.  ``target_orientation`` None solves for the position alone (``solve_ik``'s law and
        defaults: damping 1.0, error_damping 0); ``[N, 4]`` quaternions ask for the pose (``solve_ik_pose``'s law and defaults:
        damping 0.03, error_damping 0.01), ``align_axis`` as there.  ``starts``: an int S in 1, 2, 4, 8, 16, 32, 64 (the table
        ``scene.ik_start_table(S, seed)``, kept on the device per (S, seed)), a ``[S, 6]`` tensor shared by all envs or an
        ``[N, S, 6]`` tensor of each env's own; ``q_init`` (``[N, 6]``) replaces start 0 of every env.  The winner of an env is the
        smallest (not converged, cost, start index): cost = |q - q_ref|² for a converged start (``q_ref`` ``[N, 6]``; None = the
        env's start 0), the error left for the others.  ``policy`` "best": every start runs to its end; "first": an env stops at
        the first convergence check in which one of its starts converges (the shorter wave time).
        Returns a dict of device tensors, the winner's: ``q`` [N, 6], ``residual`` [N], ``angle`` [N] (0 for the position task),
        ``iterations`` [N] int32, ``start`` [N] int32 (its start index), ``converged`` [N] int32 (how many of the env's starts
        converged; 0: none did); with ``return_all`` also every start's ``all_q`` [N, S, 6], ``all_residual``, ``all_angle`` and
        ``all_iterations`` [N, S].  ``out`` may carry preallocated tensors under the same keys.  Never synchronises."""
        self._check_handle()
        n = self.num_envs
        pose = target_orientation is not None
        if align_axis is not None and not pose:
            raise AssertionError("align_axis goes with a target_orientation")
        task = _lib.IK_TASK_POSITION if not pose else (_lib.IK_TASK_POSE if align_axis is None else _lib.IK_TASK_AXIS)
        p = _lib.PnrIkMultiParams()
        self._chk(self.lib.pnr_ik_multi_params_default(p, task))
        if policy not in ("best", "first"):
            raise AssertionError(f'policy must be "best" or "first", got {policy!r}')
        p.policy = _lib.IK_MULTI_FIRST if policy == "first" else _lib.IK_MULTI_BEST
        S, table, p.starts_per_env = self._ik_starts(starts, seed)
        p.num_starts, p.link, p.max_iterations = S, int(link), int(max_iterations)
        if local_point is not None:
            for k in range(3):
                p.local_point[k] = float(local_point[k])
        if align_axis is not None:
            for k in range(3):
                p.local_axis[k] = float(align_axis[k])
        if damping is not None:
            p.damping = float(damping)
        if error_damping is not None:
            p.error_damping = float(error_damping)
        p.orientation_weight, p.max_step = float(orientation_weight), float(max_step)
        p.tolerance, p.angle_tolerance = float(tolerance), float(angle_tolerance)
        quat = None if not pose else self._in(target_orientation, (n, 4), torch.float32, "target_orientation")
        tgt = None if target is None else self._in(target, (n, 3), torch.float32, "target")
        qi = None if q_init is None else self._in(q_init, (n, 6), torch.float32, "q_init")
        qr = None if q_ref is None else self._in(q_ref, (n, 6), torch.float32, "q_ref")
        i32 = torch.int32
        res = self._asked(out, (("q", True, (n, 6), torch.float32), ("residual", True, (n,), torch.float32),
                                ("angle", True, (n,), torch.float32), ("iterations", True, (n,), i32), ("start", True, (n,), i32),
                                ("converged", True, (n,), i32), ("all_q", return_all, (n, S, 6), torch.float32),
                                ("all_residual", return_all, (n, S), torch.float32), ("all_angle", return_all, (n, S), torch.float32),
                                ("all_iterations", return_all, (n, S), i32)), "")
        b = _lib.PnrIkMultiBuffers()
        b.struct_size = C.sizeof(_lib.PnrIkMultiBuffers)
        for name, t in (("target_pos", tgt), ("target_quat", quat), ("starts", table), ("q_init", qi), ("q_ref", qr), ("q_out", res["q"]),
                        ("residual_out", res["residual"]), ("angle_out", res["angle"]), ("iterations_out", res["iterations"]),
                        ("start_out", res["start"]), ("converged_out", res["converged"]), ("all_q", res.get("all_q")),
                        ("all_residual", res.get("all_residual")), ("all_angle", res.get("all_angle")),
                        ("all_iterations", res.get("all_iterations"))):
            setattr(b, name, None if t is None else t.data_ptr())
        self._chk(self.lib.pnr_solve_ik_multi(self._h, p, b, self._stream()))
        return res

    def _ik_starts(self, starts, seed):
        """``solve_ik_multi``'s ``starts`` argument as (S, the table on the device, is it per env)."""
        n = self.num_envs
        if isinstance(starts, (int, np.integer)):
            S = int(starts)
            if S not in _lib.IK_MULTI_STARTS:
                raise AssertionError(f"starts must be one of {_lib.IK_MULTI_STARTS}, got {S}")
            tables = self.__dict__.setdefault("_ik_start_tables", {})
            if (S, int(seed)) not in tables:
                from .scene import ik_start_table
                tables[(S, int(seed))] = torch.from_numpy(ik_start_table(S, seed)).to(self.device)
            return S, tables[(S, int(seed))], 0
        shape = tuple(starts.shape)
        S = int(shape[-2]) if len(shape) in (2, 3) else 0
        if S not in _lib.IK_MULTI_STARTS:
            raise AssertionError(f"starts must be [S, 6] or [N, S, 6] with S one of {_lib.IK_MULTI_STARTS}, got {shape}")
        return S, self._in(starts, (S, 6) if len(shape) == 2 else (n, S, 6), torch.float32, "starts"), int(len(shape) == 3)

    def own_joints(self):
        """The env's own joint positions as a new float32 ``[N, 6]`` device tensor, read from the state on the device: dynamics
        mode the simulated q, kinematic mode r.  Never synchronises."""
        if self.engine_config.mode == "dynamic":
            return self.get_dyn_state()[0:6].t().contiguous()
        return self.get_state()[12:18].view(torch.float32).t().contiguous()

    def solve_ik_path(self, waypoints, orientations=None, substeps=8, starts=1, q_init=None, from_current=False, q_ref=None,
                      align_axis=None, link=10, local_point=None, max_iterations=32, track_iterations=8, damping=None,
                      error_damping=None, orientation_weight=10.0, max_step=0.5, tolerance=1e-3, angle_tolerance=1e-3, seed=0,
                      path=True, profile=False, return_all=False, winner_rows=0, out=None):
        """Cartesian path inverse kinematics for every env (pnr_solve_ik_path): the joint path on which ``local_point`` of ``link``
        follows a piecewise-linear path in the WORLD — PyBullet users' loop of ``calculateInverseKinematics(...,
        currentPositions=previous)`` over interpolated targets, in one call.

        ``waypoints``: float32 ``[K, 3]`` (one path for all envs) or ``[N, K, 3]``, K <= 256; ``orientations`` None (the position
        task, ``solve_ik``'s law and defaults) or ``[K, 4]`` / ``[N, K, 4]`` quaternions x, y, z, w (the pose task, ``solve_ik_pose``'s
        law and defaults; ``align_axis`` as there).  With M = ``substeps`` (1 .. 64) there are C = 1 + (K - 1) M configurations:
        waypoint 0, then on segment i from a to b the targets a + (j / M)(b - a), j = 1 .. M (j = M: b itself), the orientation by the
        shortest-arc normalised lerp.  Configuration c is one solve from the joints configuration c - 1 ended at, with at most
        ``track_iterations`` iterations (configuration 0: from the start, ``max_iterations``).  A configuration is reached when
        its pose is within ``tolerance`` (and ``angle_tolerance``); a start stops at the first that is not (``fail_at``), and
        its later rows are copies of that row.  ``starts`` as in ``solve_ik_multi`` (an int S, ``[S, 6]``, ``[N, S, 6]``); ``q_init``
        ``[N, 6]`` replaces start 0; ``from_current=True`` puts the env's own joints there (``own_joints()``; an error together
        with ``q_init``).  Per env the winner is the tracked start of the least travel (sum over the path of |dq_j|, plus
        |q_0 - q_ref| with ``q_ref`` ``[N, 6]``), else the start that got farthest.

        Returns a dict of device tensors: ``summary`` ``[N, 8]`` and its columns as views or small casts: ``tracked`` (bool),
        ``fail_at`` (int64, -1: none), ``max_residual``, ``max_angle`` (the largest over the configurations up to ``fail_at``),
        ``travel``, ``max_jump`` (the largest single joint move between two configurations: a branch flip shows here), ``start``
        (int64: the winner's), ``tracked_starts`` (int64); ``q_path`` ``[N, C, 6]`` unless ``path=False``; with ``profile``
        ``residual``, ``angle`` ``[N, C]`` and ``iterations`` ``[N, C]`` int32; with ``return_all`` ``all_summary`` ``[N, S, 4]`` (per start:
        tracked, fail_at, travel, max_jump).  ``winner_rows``: how the winner's rows are written under S > 1 (``_lib.IK_PATH_ROWS_*``;
        the same bits for every value).  ``out`` may carry preallocated ``summary`` / ``q_path`` / ``residual`` / ``angle`` /
        ``iterations`` / ``all_summary`` tensors, written in place.  Never synchronises.

        The two follow-ups::

            res = env.solve_ik_path(line, substeps=8, from_current=True)
            free = env.path_clearance(res["q_path"], substeps=1)["free"]        # C <= 256: is the joint path clear of the bodies?
            for c in range(res["q_path"].shape[1]):                             # .. and the motors follow it row by row
                env.world_step(motor_targets=res["q_path"][:, c])
        """
        self._check_handle()
        n = self.num_envs
        pose = orientations is not None
        if align_axis is not None and not pose:
            raise AssertionError("align_axis goes with orientations")
        if from_current and q_init is not None:
            raise AssertionError("from_current puts the env's own joints in as q_init: give one of the two")
        task = _lib.IK_TASK_POSITION if not pose else (_lib.IK_TASK_POSE if align_axis is None else _lib.IK_TASK_AXIS)
        p = _lib.PnrIkPathParams()
        self._chk(self.lib.pnr_ik_path_params_default(p, task))

        def way(t, width, name):
            if not isinstance(t, torch.Tensor):
                t = torch.as_tensor(np.asarray(t), dtype=torch.float32)
            if t.dim() not in (2, 3) or t.shape[-1] != width or (t.dim() == 3 and t.shape[0] != n):
                raise AssertionError(f"{name} must have shape (K, {width}) or ({n}, K, {width}), got {tuple(t.shape)}")
            return self._in(t, tuple(t.shape), torch.float32, name)

        wp = way(waypoints, 3, "waypoints")
        wq = way(orientations, 4, "orientations") if pose else None
        if pose and tuple(wq.shape[:-1]) != tuple(wp.shape[:-1]):
            raise AssertionError(f"orientations {tuple(wq.shape)} do not go with waypoints {tuple(wp.shape)}")
        S, table, p.starts_per_env = self._ik_starts(starts, seed)
        p.num_starts, p.n_waypoints, p.waypoints_per_env, p.substeps = S, int(wp.shape[-2]), int(wp.dim() == 3), int(substeps)
        p.link, p.max_iterations, p.track_iterations, p.winner_rows = int(link), int(max_iterations), int(track_iterations), int(winner_rows)
        if local_point is not None:
            for k in range(3):
                p.local_point[k] = float(local_point[k])
        if align_axis is not None:
            for k in range(3):
                p.local_axis[k] = float(align_axis[k])
        if damping is not None:
            p.damping = float(damping)
        if error_damping is not None:
            p.error_damping = float(error_damping)
        p.orientation_weight, p.max_step = float(orientation_weight), float(max_step)
        p.tolerance, p.angle_tolerance = float(tolerance), float(angle_tolerance)
        qi = self.own_joints() if from_current else (None if q_init is None else self._in(q_init, (n, 6), torch.float32, "q_init"))
        qr = None if q_ref is None else self._in(q_ref, (n, 6), torch.float32, "q_ref")
        configs = 1 + (p.n_waypoints - 1) * p.substeps
        i32 = torch.int32
        res = self._asked(out, (("summary", True, (n, _lib.IK_PATH_SUMMARY_DIM), torch.float32), ("q_path", path, (n, max(configs, 1), 6), torch.float32),
                                ("residual", profile, (n, max(configs, 1)), torch.float32), ("angle", profile, (n, max(configs, 1)), torch.float32),
                                ("iterations", profile, (n, max(configs, 1)), i32), ("all_summary", return_all, (n, S, 4), torch.float32)), "")
        b = _lib.PnrIkPathBuffers()
        b.struct_size = C.sizeof(_lib.PnrIkPathBuffers)
        for name, t in (("waypoint_pos", wp), ("waypoint_quat", wq), ("starts", table), ("q_init", qi), ("q_ref", qr),
                        ("summary", res["summary"]), ("q_path", res.get("q_path")), ("residual_path", res.get("residual")),
                        ("angle_path", res.get("angle")), ("iterations_path", res.get("iterations")), ("all_summary", res.get("all_summary"))):
            setattr(b, name, None if t is None else t.data_ptr())
        self._chk(self.lib.pnr_solve_ik_path(self._h, p, b, self._stream()))
        sm = res["summary"]
        res.update(tracked=sm[:, 0] > 0, fail_at=sm[:, 1].long(), max_residual=sm[:, 2], max_angle=sm[:, 3], travel=sm[:, 4],
                   max_jump=sm[:, 5], start=sm[:, 6].long(), tracked_starts=sm[:, 7].long())
        return res

    @staticmethod
    def _limits(p_field, value, name):
        """a scalar or six numbers into a params struct's double[6]"""
        v = np.asarray(value.detach().cpu().numpy() if isinstance(value, torch.Tensor) else value, dtype=np.float64)
        if v.ndim == 0:
            v = np.full(6, float(v))
        if v.shape != (6,):
            raise AssertionError(f"{name} must be a number or six of them, got shape {v.shape}")
        for j in range(6):
            p_field[j] = float(v[j])

    def _timed_path(self, q_path):
        n = self.num_envs
        if not isinstance(q_path, torch.Tensor):
            q_path = torch.as_tensor(np.asarray(q_path), dtype=torch.float32)
        if q_path.dim() not in (2, 3) or q_path.shape[-1] != 6 or (q_path.dim() == 3 and q_path.shape[0] != n):
            raise AssertionError(f"q_path must have shape (C, 6) or ({n}, C, 6), got {tuple(q_path.shape)}")
        return self._in(q_path, tuple(q_path.shape), torch.float32, "q_path")

    def retime_path(self, q_path, v_max, a_max, tau_max=None, dt=None, steps=None, t0=0.0, profile=True, out=None):
        """Time parameterisation of every env's joint path, one call (pnr_retime_path): when the arm should be at which row of
        ``q_path``, rest to rest, as fast as the limits allow — time-optimal path parameterisation by reachability analysis (a
        backward pass of controllable sets, a greedy forward pass) on the path's own grid; the law is include/pioneer_amd.h's.

        ``q_path``: float32 ``[C, 6]`` (one path for all envs) or ``[N, C, 6]``, 3 <= C <= 256 — what ``solve_ik_path`` returns and
        ``path_clearance`` takes.  ``v_max``, ``a_max``: the joints' velocity and acceleration limits, a number or six; ``tau_max``
        (None: no torque rows) the joint-torque limits: the rows ``|M(q) q̈ + C q̇ + G| <= tau_max`` on the model ``inverse_dynamics``
        evaluates (dynamics mode: each env's link scales and the config's gravity), so the answer differs per env and payload.

        Returns a dict of device tensors: ``summary`` ``[N, 8]`` and its columns as views or small casts — ``feasible`` (bool),
        ``duration`` (+inf when infeasible), ``fail_at`` (int64 grid index, -1), ``reason`` (int64, ``_lib.RETIME_*``: empty
        controllable set, stuck, not finite), ``max_sdot``, ``utilisation`` (the largest row value over its limit: 1 up to float32
        where a limit is active) — and with ``profile`` ``times`` and ``sdot2`` ``[N, C]`` (t_k and ṡ² at the grid points).  With
        ``steps`` (an int, see ``scene.steps_for``) also ``targets`` ``[N, steps, 12]``: the rows q | q̇ at t0 + (i + 1) dt,
        ``dt`` defaulting to the handle's timestep x frame_skip (one world step), each what ``world_step(motor_targets=…)``
        takes; past the end they hold the last point, and an infeasible env's rows hold the first.  ``out`` may carry
        preallocated ``summary`` / ``times`` / ``sdot2`` / ``targets`` tensors, written in place.  The torque rows' workspace is
        cached per (C, N).  Never synchronises.  A coarse grid can make the arm stop inside the path::

            res = env.solve_ik_path(line, substeps=8, from_current=True)
            timed = env.retime_path(res["q_path"], 2.0, 10.0, tau_max=700.0, steps=240)
            for i in range(240):
                env.world_step(motor_targets=timed["targets"][:, i])
        """
        self._check_handle()
        n = self.num_envs
        qp = self._timed_path(q_path)
        p = _lib.PnrRetimeParams()
        self._chk(self.lib.pnr_retime_params_default(p))
        p.n_points, p.path_per_env = int(qp.shape[-2]), int(qp.dim() == 3)
        self._limits(p.v_max, v_max, "v_max")
        self._limits(p.a_max, a_max, "a_max")
        if tau_max is not None:
            p.flags = _lib.RETIME_TORQUE
            self._limits(p.tau_max, tau_max, "tau_max")
        Cn = p.n_points
        need = profile or steps is not None
        res = self._asked(out, (("summary", True, (n, _lib.RETIME_SUMMARY_DIM), torch.float32), ("times", need, (n, Cn), torch.float32),
                                ("sdot2", need, (n, Cn), torch.float32)), "")
        b = _lib.PnrRetimeBuffers()
        b.struct_size = C.sizeof(_lib.PnrRetimeBuffers)
        ws = None
        if tau_max is not None:
            nbytes = C.c_uint64(0)
            self._chk(self.lib.pnr_retime_workspace_bytes(self._h, p, C.byref(nbytes)))
            cache = self.__dict__.setdefault("_retime_workspaces", {})
            if (Cn, n) not in cache:
                cache[(Cn, n)] = self._new((int(nbytes.value) // 4,))
            ws = cache[(Cn, n)]
        for name, t in (("q_path", qp), ("workspace", ws), ("summary", res["summary"]), ("times", res.get("times")), ("sdot2", res.get("sdot2"))):
            setattr(b, name, None if t is None else t.data_ptr())
        self._chk(self.lib.pnr_retime_path(self._h, p, b, self._stream()))
        sm = res["summary"]
        res.update(feasible=sm[:, 0] > 0, duration=sm[:, 1], fail_at=sm[:, 2].long(), reason=sm[:, 3].long(), max_sdot=sm[:, 4],
                   utilisation=sm[:, 5])
        if steps is not None:
            res["targets"] = self.sample_trajectory(qp, res["times"], res["sdot2"], sm, steps, dt=dt, t0=t0,
                                                    out=None if out is None else out.get("targets"))
        return res

    def sample_trajectory(self, q_path, times, sdot2, summary, steps, dt=None, t0=0.0, out=None):
        """Another window of an already timed path (pnr_sample_trajectory): float32 ``[N, steps, 12]`` rows q | q̇ at
        t0 + (i + 1) dt, i = 0 .. steps - 1, from ``retime_path``'s ``times``, ``sdot2`` and ``summary`` of the same ``q_path``.
        ``dt`` None: the handle's timestep x frame_skip.  Windows t0 = 0, steps dt, 2 steps dt, .. tile the trajectory.  Past
        the duration a row is the last point at rest; an infeasible env's rows are the first point at rest.  Never synchronises."""
        self._check_handle()
        n = self.num_envs
        qp = self._timed_path(q_path)
        Cn = int(qp.shape[-2])
        p = _lib.PnrTrajSampleParams()
        self._chk(self.lib.pnr_traj_sample_params_default(p))
        p.n_points, p.path_per_env, p.n_samples = Cn, int(qp.dim() == 3), int(steps)
        p.t0 = float(t0)
        p.dt = float(self._c_cfg.timestep * self._c_cfg.frame_skip if dt is None else dt)
        tm = self._in(times, (n, Cn), torch.float32, "times")
        xs = self._in(sdot2, (n, Cn), torch.float32, "sdot2")
        sm = self._in(summary, (n, _lib.RETIME_SUMMARY_DIM), torch.float32, "summary")
        res = self._out(out, "targets", (n, max(int(steps), 1), 12))
        self._chk(self.lib.pnr_sample_trajectory(self._h, p, _ptr(qp), _ptr(tm), _ptr(xs), _ptr(sm), _ptr(res), self._stream()))
        return res

    def target_reachable(self, within=None, starts=None):
        """bool ``[N]``: can the pointer get within ``within`` (default the config's ``done_distance``) of the env's own target
        without leaving the joint limits?  ``solve_ik()`` from the rest pose with all defaults; about 3 % of the reference's
        target box (its far corners) cannot be reached, and such an episode can only end at the time limit.  True is exact; False
        means "not reached from the rest pose", which for about one target in a hundred is a local minimum of that start.
        ``starts`` (as ``solve_ik_multi``'s): the best of that many starts instead; False then means "from none of them"."""
        within = float(self.config.done_distance if within is None else within)
        if starts is not None:
            return self.solve_ik_multi(starts=starts, policy="first")["residual"] <= within
        return self.solve_ik()[1] <= within

    def render_frames(self, render_config=None, joint_state=None, bodies=None, rgb=True, depth=False, segmentation=False, out=None,
                      light_direction=(0.4, 0.2, 1.0), ambient=0.45, diffuse=0.55, background=(1.0, 1.0, 1.0), target_rgba=None,
                      body_positions=None, camera_link=None, cameras=None):
        """render('rgb_array') of every env in one launch (bullet_env.py:156-185 -> getCameraImage; pnr_render): the URDF's 14
        visual shapes in their materials' colours, posed by each env's joints, the translucent target sphere and static bodies,
        seen by the camera of ``render_config`` (a RenderConfig, default RenderConfig(); render.view_matrix, its fov, near, far).

        Returns a dict of device tensors, those asked for: ``rgb`` uint8 [N, H, W, 3], ``depth`` float32 [N, H, W] (eye depth
        along the view axis, +inf where nothing is hit), ``seg`` uint8 [N, H, W] (``_lib.SEG_*``: 0 background, 1 + link index,
        12 the target, 13 + body index, 21 the moving sphere).  ``joint_state``: as ``link_states`` (None = the handle's own
        joints).  ``bodies``: None draws ``engine_config.scene`` in the URDF's obstacle_mat colour; else a sequence of (SceneBody,
        rgba) pairs.  ``body_positions`` (float32 ``[N, len(bodies), 3]``): a world position per env in place of each body's own, as
        in ``contacts`` (pnr_render_bodies); after ``set_body_queries(render=True)`` every env with a moving sphere shows it.
        Shading: c = clamp(rgb (ambient + diffuse max(0, n . l)), 0, 1) with the defaults light_direction (0.4, 0.2, 1.0) (towards
        the light, world frame: from above, on the default camera's side), ambient 0.45, diffuse 0.55, a white background;
        ``target_rgba`` defaults to the env's PioneerKinematicConfig.target_rgba.  ``out`` may carry preallocated ``rgb`` /
        ``depth`` / ``seg`` tensors, written in place.  Never synchronises.

        A camera per env (pnr_render_cameras; getCameraImage with a view matrix per env): ``cameras``, a float32 tensor ``[7]``
        (one row for all envs) or ``[N, 7]`` on the env's device (host values are copied), each row position | quaternion
        (x, y, z, w) of the camera frame (x right, y up, looking along -z) in its parent frame (``render.camera_pose``,
        ``render.look_at_cameras``); ``camera_link``, the parent frame: None the world, else an int 0 .. 10 or a name of
        ``LINK_NAMES``, that link of EACH env (an eye-in-hand camera; the link's pose follows the joints the arm is drawn from).
        ``camera_link`` alone mounts ``render_config``'s camera pose on the link; its fov, near, far and size hold in every case.
        A camera inside a shape sees that shape's far face: keep a wrist camera outside its link's shapes.  With both left out
        the call is the shared-camera call above."""
        from . import render as _render
        from .config import RenderConfig
        self._check_handle()
        cfg = render_config or RenderConfig()
        n, H, W = self.num_envs, int(cfg.render_height), int(cfg.render_width)
        if bodies is None:
            bodies = [(b, _render.OBSTACLE_RGBA) for b in self.engine_config.scene]
        bodies = list(bodies)
        if len(bodies) > _lib.MAX_SCENE:
            raise AssertionError(f"at most {_lib.MAX_SCENE} bodies can be drawn, got {len(bodies)}")
        p = _lib.PnrRenderParams()
        p.struct_size = C.sizeof(_lib.PnrRenderParams)
        p.width, p.height, p.n_bodies = W, H, len(bodies)
        V = _render.view_matrix(cfg)
        for k, v in enumerate(np.asarray(V, dtype=np.float64).reshape(-1)):
            p.view[k] = float(v)
        p.fov_y, p.near_clip, p.far_clip = float(cfg.projection_fov), float(cfg.projection_near), float(cfg.projection_far)
        for k in range(3):
            p.light_direction[k] = float(light_direction[k])
            p.background[k] = float(background[k])
        p.ambient, p.diffuse = float(ambient), float(diffuse)
        trgba = self.config.target_rgba if target_rgba is None else target_rgba
        for k in range(4):
            p.target_rgba[k] = float(trgba[k])
        for i, (b, rgba) in enumerate(bodies):
            fill_scene_body(p.bodies[i], b, f"body {i}")
            for k in range(4):
                p.body_rgba[i][k] = float(rgba[k])
        js = self._joints(joint_state)
        res = self._asked(out, (("rgb", rgb, (n, H, W, 3), torch.uint8), ("depth", depth, (n, H, W), torch.float32),
                                ("seg", segmentation, (n, H, W), torch.uint8)), "render_frames: ask for at least one of rgb, depth, segmentation")
        if camera_link is not None or cameras is not None:
            if isinstance(camera_link, str) and camera_link not in LINK_NAMES:
                raise AssertionError(f"render_frames: no link named {camera_link!r}")
            link = -1 if camera_link is None else (LINK_NAMES.index(camera_link) if isinstance(camera_link, str) else int(camera_link))
            cams = None
            if cameras is not None:
                if not isinstance(cameras, torch.Tensor):
                    cameras = torch.as_tensor(np.asarray(cameras), dtype=torch.float32)
                if tuple(cameras.shape) not in ((7,), (n, 7)):
                    raise AssertionError(f"cameras must have shape (7,) or ({n}, 7), got {tuple(cameras.shape)}")
                cams = self._in(cameras, tuple(cameras.shape), torch.float32, "cameras")
            bp = None if body_positions is None else self._in(body_positions, (n, len(bodies), 3), torch.float32, "body_positions")
            self._chk(self.lib.pnr_render_cameras(self._h, _ptr(js), p, _ptr(bp), link, _ptr(cams), int(cams is not None and cams.dim() == 2),
                                                  _ptr(res.get("rgb")), _ptr(res.get("depth")), _ptr(res.get("seg")), self._stream()))
            return res
        if body_positions is None and not (self._body_queries or {}).get("render"):
            self._chk(self.lib.pnr_render(self._h, _ptr(js), p, _ptr(res.get("rgb")), _ptr(res.get("depth")), _ptr(res.get("seg")),
                                          self._stream()))
            return res
        bp = None if body_positions is None else self._in(body_positions, (n, len(bodies), 3), torch.float32, "body_positions")
        self._chk(self.lib.pnr_render_bodies(self._h, _ptr(js), p, _ptr(bp), _ptr(res.get("rgb")), _ptr(res.get("depth")),
                                             _ptr(res.get("seg")), self._stream()))
        return res

    def collision_bodies(self):
        """The env's own collision world as a body list, in the order that is the body index of ``contacts()``: the ``ground_z``
        plane (normal +z) if set, the obstacle box (``obstacle_position`` / ``obstacle_half_extents``) if set, then
        ``engine_config.scene`` in its own order."""
        from .config import scene_box, scene_plane
        ec = self.engine_config
        bodies = []
        if ec.ground_z == ec.ground_z:
            bodies.append(scene_plane((0.0, 0.0, 1.0), (0.0, 0.0, float(ec.ground_z))))
        if all(float(h) > 0 for h in ec.obstacle_half_extents):
            bodies.append(scene_box(ec.obstacle_half_extents, ec.obstacle_position))
        return bodies + list(ec.scene)

    def contacts(self, joint_state=None, bodies=None, body_positions=None, points=True, summary=True, joint_torques=False, out=None):
        """getContactPoints / getClosestPoints of every env, one launch (pnr_get_contacts): the arm's 23 contact sample spheres
        (``_lib.CONTACT_SAMPLES``; ``scene.CONTACT_SAMPLE_LINKS`` names their URDF links, sample 22 is the pointer) against static
        bodies, surface to surface.  Works in either mode.  Returns a dict of device tensors, those asked for:

        ``points`` float32 ``[N, 23, 9]``: per sample, against its nearest body, the signed distance (< 0: penetrating; +inf
        without bodies), the unit world normal on the body towards the sample [3], the world position on the sample's surface
        [3] (the position on the body is that minus distance x normal), the body index (-1 without bodies) and that body's
        normal force max(0, kp depth - kd v.n);
        ``summary`` float32 ``[N, 4]``: the smallest distance, its sample, its body, the number of penetrating samples;
        ``joint_torques`` float32 ``[N, 6]``: the joint torques of all contact forces, sum_s J_s^T F_s over all bodies — given to
        ``world_step(joint_torques=...)`` of a contact-free env they reproduce a step with contacts.

        ``bodies``: a sequence of SceneBody (config.scene_plane / scene_box / scene_sphere), at most 8; the BODY INDEX is the
        position in it.  None = the env's own collision world, ``collision_bodies()``: the ``ground_z`` plane if set, the
        obstacle box if set, then ``engine_config.scene``.  ``body_positions`` (float32 ``[N, len(bodies), 3]``): a world position
        per env in place of each body's own (orientation and size stay shared): the per-env obstacle.  ``joint_state``: as
        ``link_states`` (None = the handle's own joints).  The gains are the config's ``contact_kp`` / ``contact_kd``; the
        pointer's radius its ``pointer_radius``.  After ``set_body_queries(contacts=True)`` every env with a moving sphere reports
        it as one more body, index ``_lib.MAX_SCENE`` (8), under the step's arm-sphere law with the sphere's own velocity and
        radius (it loses a distance tie to a body of ``bodies``; with no ``bodies`` it is the nearest body of its env).  ``out`` may carry preallocated ``points`` / ``summary`` / ``joint_torques``
        tensors, written in place.  Never synchronises."""
        self._check_handle()
        n = self.num_envs
        bodies = self.collision_bodies() if bodies is None else list(bodies)
        if len(bodies) > _lib.MAX_SCENE:
            raise AssertionError(f"at most {_lib.MAX_SCENE} bodies can be queried, got {len(bodies)}")
        p = _lib.PnrContactParams()
        self._chk(self.lib.pnr_contact_params_default(p))
        p.n_bodies = len(bodies)
        p.contact_kp, p.contact_kd = float(self.engine_config.contact_kp), float(self.engine_config.contact_kd)
        for i, b in enumerate(bodies):
            fill_scene_body(p.bodies[i], b, f"body {i}")
        js = self._joints(joint_state)
        bp = None if body_positions is None else self._in(body_positions, (n, len(bodies), 3), torch.float32, "body_positions")
        res = self._asked(out, (("points", points, (n, _lib.CONTACT_SAMPLES, _lib.CONTACT_DIM), torch.float32), ("summary", summary, (n, 4), torch.float32),
                                ("joint_torques", joint_torques, (n, 6), torch.float32)), "contacts: ask for at least one of points, summary, joint_torques")
        self._chk(self.lib.pnr_get_contacts(self._h, _ptr(js), p, _ptr(bp), _ptr(res.get("points")), _ptr(res.get("summary")),
                                            _ptr(res.get("joint_torques")), self._stream()))
        return res

    def path_clearance(self, waypoints, substeps=8, from_current=False, bodies=None, body_positions=None, margin=0.0, samples=None,
                       profile=False, lanes_per_env=0, out=None):
        """Sweeps every env's arm along a joint path, one launch (pnr_path_clearance): can env k move from waypoint to waypoint
        without touching its bodies?  A SAMPLED check: only the configurations below are looked at (``scene.path_substeps``
        chooses ``substeps`` for a joint step).

        ``waypoints``: float32 ``[K, 6]`` (one path for all envs) or ``[N, K, 6]`` (a path per env), K <= 256; None with
        ``from_current`` (the env where it stands).  ``from_current``: the env's own joints (dynamics mode the simulated q,
        kinematic mode r) are waypoint 0 in front of them.  With W waypoints and M = ``substeps`` (1 .. 64) there are
        C = 1 + (W - 1) M configurations: waypoint 0, then on segment i from a to b the configurations a + (j / M)(b - a),
        j = 1 .. M (j = M: b itself), at the path coordinate t = i + j / M.  ``substeps=1`` looks at the waypoints alone: a set
        of candidates.  A configuration's clearance is the smallest ``contacts()`` distance over the sample spheres (``samples``:
        a sequence of sample indices 0 .. 22, None = all 23) and the bodies; ``bodies`` / ``body_positions`` as in ``contacts``
        (None = ``collision_bodies()``), and after ``set_body_queries(contacts=True)`` the env's moving sphere, standing still, is
        body ``_lib.MAX_SCENE``.  A distance that is not finite counts as -inf (a NaN waypoint makes the path not free).

        Returns a dict of device tensors, views or cheap casts of the ``[N, 8]`` ``summary`` (also returned): ``min_distance``
        (the smallest clearance over the path), ``at`` (its t; the lowest configuration on a tie), ``sample``, ``body`` (int64:
        who attains it; body -1 without bodies), ``first_hit`` (t of the first configuration with clearance < ``margin``, -1 if
        none), ``violations`` (int64: how many such), ``free`` (bool: none); with ``profile`` also ``clearance`` ``[N, C]``.
        ``lanes_per_env``: 0 (auto) or 1, 2, .. 64 lanes of a wave per env; the results are the same bits for every value.
        ``out`` may carry preallocated ``summary`` / ``clearance`` tensors, written in place.  Never synchronises."""
        self._check_handle()
        n = self.num_envs
        bodies = self.collision_bodies() if bodies is None else list(bodies)
        if len(bodies) > _lib.MAX_SCENE:
            raise AssertionError(f"at most {_lib.MAX_SCENE} bodies can be queried, got {len(bodies)}")
        p = _lib.PnrPathParams()
        self._chk(self.lib.pnr_path_params_default(p))
        wp = None
        p.n_waypoints = 0
        if waypoints is not None:
            if not isinstance(waypoints, torch.Tensor):
                waypoints = torch.as_tensor(np.asarray(waypoints), dtype=torch.float32)
            if waypoints.dim() not in (2, 3) or waypoints.shape[-1] != 6 or (waypoints.dim() == 3 and waypoints.shape[0] != n):
                raise AssertionError(f"waypoints must have shape (K, 6) or ({n}, K, 6), got {tuple(waypoints.shape)}")
            wp = self._in(waypoints, tuple(waypoints.shape), torch.float32, "waypoints")
            p.n_waypoints, p.waypoints_per_env = int(wp.shape[-2]), int(wp.dim() == 3)
        p.substeps, p.from_current, p.lanes_per_env, p.margin = int(substeps), int(bool(from_current)), int(lanes_per_env), float(margin)
        if samples is not None:
            mask = 0
            for s in samples:
                if not 0 <= int(s) < _lib.CONTACT_SAMPLES:
                    raise AssertionError(f"samples are indices 0 .. {_lib.CONTACT_SAMPLES - 1}, got {s}")
                mask |= 1 << int(s)
            p.sample_mask = mask
        p.n_bodies = len(bodies)
        for i, b in enumerate(bodies):
            fill_scene_body(p.bodies[i], b, f"body {i}")
        bp = None if body_positions is None else self._in(body_positions, (n, len(bodies), 3), torch.float32, "body_positions")
        configs = 1 + (p.n_waypoints + p.from_current - 1) * p.substeps
        res = self._asked(out, (("summary", True, (n, _lib.PATH_SUMMARY_DIM), torch.float32),
                                ("clearance", profile, (n, max(configs, 1)), torch.float32)), "")
        self._chk(self.lib.pnr_path_clearance(self._h, p, _ptr(wp), _ptr(bp), _ptr(res["summary"]), _ptr(res.get("clearance")), self._stream()))
        sm = res["summary"]
        res.update(min_distance=sm[:, 0], at=sm[:, 1], sample=sm[:, 2].long(), body=sm[:, 3].long(), first_hit=sm[:, 4],
                   violations=sm[:, 5].long(), free=sm[:, 6] > 0)
        return res

    def solve_ik_free(self, target_orientation=None, target=None, margin=0.0, bodies=None, body_positions=None, **ik_multi_args):
        """Collision-aware inverse kinematics, two launches: ``solve_ik_multi(return_all=True, policy="best")`` and ONE
        ``path_clearance`` over every start's solution as the env's waypoints with ``substeps=1``, then a small selection on the
        device.  Per env the result is the CONVERGED start nearest to ``q_ref`` (``solve_ik_multi``'s cost, |q - q_ref|^2; None =
        the env's start 0; the lowest start on a tie) whose clearance is >= ``margin``; ``free`` (bool ``[N]``) tells whether there
        was one, and where there was none the row is ``solve_ik_multi``'s own winner.  ``bodies`` / ``body_positions`` as in
        ``contacts``; every other argument goes to ``solve_ik_multi``.
        Returns ``solve_ik_multi``'s dict with ``q``, ``residual``, ``angle``, ``iterations``, ``start`` of the chosen start, and
        ``free``, ``clearance`` ``[N]`` (the chosen configuration's) and ``all_clearance`` ``[N, S]``.  Never synchronises."""
        for key in ("return_all", "policy"):
            if key in ik_multi_args:
                raise AssertionError(f"solve_ik_free sets {key} itself")
        q_ref = ik_multi_args.get("q_ref")
        res = self.solve_ik_multi(target_orientation=target_orientation, target=target, return_all=True, policy="best", **ik_multi_args)
        n, S = res["all_residual"].shape
        clr = self.path_clearance(res["all_q"], substeps=1, bodies=bodies, body_positions=body_positions, margin=margin, profile=True)["clearance"]
        tol = float(ik_multi_args.get("tolerance", 1e-3))
        conv = res["all_residual"] <= tol
        if target_orientation is not None:
            conv = conv & (res["all_angle"] <= float(ik_multi_args.get("angle_tolerance", 1e-3)))
        allq = res["all_q"]
        if q_ref is not None:
            ref = self._in(q_ref, (n, 6), torch.float32, "q_ref")
        elif ik_multi_args.get("q_init") is not None:
            ref = self._in(ik_multi_args["q_init"], (n, 6), torch.float32, "q_init")
        else:
            starts = ik_multi_args.get("starts", 8)
            if isinstance(starts, (int, np.integer)):
                ref = self._ik_start_tables[(int(starts), int(ik_multi_args.get("seed", 0)))][0].expand(n, 6)
            else:
                st = self._in(starts, tuple(starts.shape), torch.float32, "starts")
                ref = st[0].expand(n, 6) if st.dim() == 2 else st[:, 0]
        cost = ((allq - ref[:, None, :]) ** 2).sum(dim=2)
        ok = conv & (clr >= float(margin))
        cost = torch.where(ok, cost, torch.full_like(cost, float("inf")))
        pick = cost.argmin(dim=1)                       # (the first of equal costs: the lowest start)
        free = ok.any(dim=1)
        pick = torch.where(free, pick, res["start"].long())
        rows = torch.arange(n, device=self.device)
        res["q"] = torch.where(free[:, None], allq[rows, pick], res["q"])
        for key, every in (("residual", "all_residual"), ("angle", "all_angle"), ("iterations", "all_iterations")):
            res[key] = torch.where(free, res[every][rows, pick], res[key])
        res["start"] = pick.to(torch.int32)
        res["free"] = free
        res["all_clearance"] = clr
        res["clearance"] = clr[rows, pick]
        return res

    def ray_test(self, rays, parent_link=-1, hit_arm=False, hit_target=False, hit_bodies=True, bodies=None, body_positions=None,
                 joint_state=None, hits=True, fractions=False, out=None):
        """rayTest / rayTestBatch of every env, one launch (pnr_ray_test): range sensors and line-of-sight checks.  ``rays``: a
        float32 tensor ``[R, 6]`` (shared by all envs) or ``[N, R, 6]`` (per env), R <= ``_lib.MAX_RAYS``; a ray is the segment
        from ``[..., 0:3]`` to ``[..., 3:6]``, in the world frame (``parent_link=-1``) or in the frame of URDF link
        ``parent_link`` (0 .. 10, ``link_states``' index) of EACH env: a sensor mounted on the arm.  Returns a dict of device
        tensors, those asked for:

        ``hits`` float32 ``[N, R, 8]``: the hit fraction (1 on a miss, PyBullet's convention), the world hit position [3] (``to``
        on a miss), the unit outward world normal [3] (0 on a miss) and the ``_lib.SEG_*`` label as a float (0 miss, 1 + link,
        12 the target, 13 + body index);
        ``fractions`` float32 ``[N, R]``: the hit fraction alone, the tensor that goes into an observation.

        What a ray can hit: ``hit_bodies`` the static ``bodies`` (a sequence of SceneBody, at most 8, planes as half-spaces below
        their surface; None = ``collision_bodies()``, as in ``contacts()``; ``body_positions`` ``[N, len(bodies), 3]`` a world
        position per env), ``hit_arm`` the URDF's 14 visual shapes posed by the env's joints (what ``render_frames`` draws),
        ``hit_target`` the target sphere; after ``set_body_queries(rays=True)`` ``hit_bodies`` includes every env's moving sphere
        (label ``_lib.SEG_MOVING_BODY`` = 21).  Every shape is a solid; a ray that starts inside one does not hit it.  The default is
        what Bullet would hit: the reference URDF has no collision shapes.  ``joint_state``: as ``link_states`` (None = the
        handle's own joints).  ``out`` may carry preallocated ``hits`` / ``fractions`` tensors, written in place.  Never
        synchronises."""
        self._check_handle()
        n = self.num_envs
        if not isinstance(rays, torch.Tensor):
            rays = torch.as_tensor(np.asarray(rays), dtype=torch.float32)
        if rays.dim() not in (2, 3) or rays.shape[-1] != 6 or (rays.dim() == 3 and rays.shape[0] != n):
            raise AssertionError(f"rays must have shape (R, 6) or ({n}, R, 6), got {tuple(rays.shape)}")
        nr = int(rays.shape[-2])
        if not 1 <= nr <= _lib.MAX_RAYS:
            raise AssertionError(f"between 1 and {_lib.MAX_RAYS} rays per env, got {nr}")
        rays = self._in(rays, tuple(rays.shape), torch.float32, "rays")
        bodies = self.collision_bodies() if bodies is None else list(bodies)
        if len(bodies) > _lib.MAX_SCENE:
            raise AssertionError(f"at most {_lib.MAX_SCENE} bodies can be queried, got {len(bodies)}")
        p = _lib.PnrRayParams()
        self._chk(self.lib.pnr_ray_params_default(p))
        p.n_rays, p.rays_per_env, p.parent_link = nr, int(rays.dim() == 3), int(parent_link)
        p.hit_mask = (_lib.RAY_HIT_BODIES if hit_bodies else 0) | (_lib.RAY_HIT_ARM if hit_arm else 0) | (_lib.RAY_HIT_TARGET if hit_target else 0)
        p.n_bodies = len(bodies)
        for i, b in enumerate(bodies):
            fill_scene_body(p.bodies[i], b, f"body {i}")
        js = self._joints(joint_state)
        bp = None if body_positions is None else self._in(body_positions, (n, len(bodies), 3), torch.float32, "body_positions")
        res = self._asked(out, (("hits", hits, (n, nr, _lib.RAY_DIM), torch.float32), ("fractions", fractions, (n, nr), torch.float32)),
                          "ray_test: ask for at least one of hits, fractions")
        self._chk(self.lib.pnr_ray_test(self._h, _ptr(js), p, _ptr(rays), _ptr(bp), _ptr(res.get("hits")), _ptr(res.get("fractions")),
                                        self._stream()))
        return res

    def observe(self, out=None):
        """observe() without stepping (pioneer_knm_env.py:184-211)."""
        self._check_handle()
        obs = self._out(out, "out", self.obs_shape)
        self._chk(self.lib.pnr_observe(self._h, _ptr(obs), self._stream()))
        return obs

    # -- raw state ------------------------------------------------------------------------
    def get_state(self):
        """Planar state words uint32-as-int32 ``[24, N]`` (see include/pioneer_amd.h)."""
        self._check_handle()
        w = torch.empty((_lib.STATE_WORDS, self.num_envs), dtype=torch.int32, device=self.device)
        self._chk(self.lib.pnr_get_state(self._h, _ptr(w), self._stream()))
        return w

    def set_state(self, words):
        self._check_handle()
        w = self._in(words, (_lib.STATE_WORDS, self.num_envs), torch.int32, "words")
        self._chk(self.lib.pnr_set_state(self._h, _ptr(w), self._stream()))
        torch.cuda.current_stream(self.device).synchronize()  # `w` may be a temporary

    def get_dyn_state(self):
        self._check_handle()
        w = torch.empty((_lib.DYN_STATE_WORDS, self.num_envs), dtype=torch.float32, device=self.device)
        self._chk(self.lib.pnr_get_dyn_state(self._h, _ptr(w), self._stream()))
        return w

    def set_dyn_state(self, words):
        self._check_handle()
        w = self._in(words, (_lib.DYN_STATE_WORDS, self.num_envs), torch.float32, "words")
        self._chk(self.lib.pnr_set_dyn_state(self._h, _ptr(w), self._stream()))
        torch.cuda.current_stream(self.device).synchronize()

    def state_dict(self):
        """Decoded state (numpy, host): a, v, r [N,6]; target [N,3]; potential, step_index, episode [N]; with a moving sphere
        enabled (``set_body``) also body [N,8], with the grip enabled (``set_body_grip``) also grip [N,4]."""
        w = self.get_state().cpu().numpy().view(np.uint32)
        f = w.view(np.float32)
        d = dict(a=f[0:6].T.copy(), v=f[6:12].T.copy(), r=f[12:18].T.copy(), target=f[18:21].T.copy(),
                 potential=f[21].copy(), step_index=w[22].copy(), episode=w[23].copy())
        if self._body_on:
            d["body"] = self.body_state().cpu().numpy()
        if self._grip_on:
            d["grip"] = self.body_grip().cpu().numpy()
        return d

    def load_state_dict(self, d):
        """``state_dict``'s inverse: the command state, and the spheres' where the dict carries a ``body`` key (which needs
        ``set_body`` first: the params are not part of the state), and every env's grip word ``max_force`` where it carries a
        ``grip`` key (``set_body_grip`` first; the reported force restarts at zero)."""
        w = np.zeros((_lib.STATE_WORDS, self.num_envs), dtype=np.uint32)
        f = w.view(np.float32)
        f[0:6], f[6:12], f[12:18], f[18:21] = (np.asarray(d[k], dtype=np.float32).T for k in ("a", "v", "r", "target"))
        f[21] = d["potential"]
        w[22], w[23] = d["step_index"], d["episode"]
        self.set_state(torch.from_numpy(w.view(np.int32)))
        if "body" in d:
            self.set_body_state(d["body"])
        if "grip" in d:
            self.set_body_grip(max_force=np.asarray(d["grip"])[:, 0])

    def __reduce__(self):
        """Pickled by constructor arguments (a fresh batch, like the reference's EzPickle envs);
        use get_state()/set_state() to carry the simulation state."""
        return (_rebuild_vector_env, (self._ctor,))

    def get_unwrapped(self):
        return []

    def close(self):
        if getattr(self, "_h", None) is not None:
            torch.cuda.synchronize(self.device)
            self.lib.pnr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
