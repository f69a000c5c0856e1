"""``env.scene`` / ``env.world``: the object surface the reference's demo drives (pioneer_knm_env.py:245-296 ``__main__``:
``env.scene.create_body_box / create_body_plane``, ``env.scene.rpy2quat``, ``env.scene.joints_by_name[...]`` with ``position()``,
``lower_limit / upper_limit``, ``reset_state(position, velocity)``, ``control_position / control_velocity``; ``env.world.step()``,
``env.world.step_time``) over the HIP engine.

The reference's ``Scene`` / ``Joint`` / ``World`` (bullet_scene.py:70-279) are views of a PyBullet client; here they are views of the
one-env engine batch of ``PioneerKinematicEnv``.  What maps and how:

* joints: the six revolute joints of the URDF, by the URDF's names (bullet_env.py:141-146 keeps exactly these).  The Bullet client's
  joint state is NOT the env's ``self.r / self.v`` (pioneer_knm_env.py:144-146): the env teleports its r into Bullet with velocity 0
  on every step (:148, bullet_scene.py:157-165) and nothing flows back.  So ``position() / velocity() / reset_state`` work on the
  SIMULATOR's joints and never on the env's command state:
  dynamics mode — the engine's simulated q, q̇ (``pnr_get_dyn_state``);
  kinematic mode — a [1, 12] device buffer of this Scene (q | q̇), set to (r, 0) by every ``env.step`` / ``reset_world`` — what act()
  leaves in Bullet — and advanced by ``world.step()``.  ``env.step(a)`` followed by ``env.world.step()`` therefore changes nothing.
* ``control_position / control_velocity`` (bullet_scene.py:123-155): dynamics mode: the joint's motor for ``world.step()``
  (``pnr_set_joint_motor``).  ``EngineConfig.joint_motor == "pd"``: the engine's PD motor law with this joint's targets, gains,
  force and maxVelocity; an argument left ``None`` takes the EngineConfig's value.  ``"constraint"``: Bullet's velocity-level
  constraint motor; an argument left ``None`` takes Bullet's value, and ``max_force=0`` leaves the joint free.  Kinematic mode
  has no motors (the engine says so).
* bodies: ``create_body_box / plane / sphere`` with ``mass == 0``.  The reference's arm has no ``<collision>`` shapes, so there a
  created body never touches it: in kinematic mode a body is a record (``items_by_name``), as inert as in the reference.  In dynamics
  mode a body with a collision shape becomes a static scene body of the engine (``EngineConfig.scene``; the handle is rebuilt with the
  env's state and the joints' motors carried over).  ``create_body_sphere(mass > 0, collision=True)`` on a dynamics-mode env creates
  the engine's ONE moving sphere (``PioneerVectorEnv.set_body``: a point mass with a radius, no spin — rolling is not modelled):
  ``world.step()`` moves it, its ``Item.pose() / velocity() / reset_pose()`` are engine calls (the base-item branch of
  bullet_scene.py:53-73), ``render("rgb_array")`` draws it where it is; a second one, one in kinematic mode or without a collision
  shape asserts, and so does a box or plane with ``mass > 0``.  The moving sphere is among the bodies of ``contact_points`` /
  ``closest_points`` / ``ray_test`` / ``ray_test_batch`` (``PioneerVectorEnv.set_body_queries``: the engine's queries read its state
  where it is, with its velocity in the contact force); its body id is ``body_id(item)``, one past the created static bodies'.
* ``control_torque(torque)`` (setJointMotorControl2 with TORQUE_CONTROL; the reference's Joint has no such method, Bullet does):
  dynamics mode with the PD motors: the joint's torque for the next ``world.step()`` alone (``pnr_world_step_torques``), next to its
  motor; kinematic mode and ``joint_motor == "constraint"`` raise.
* ``apply_force(force, position=None, frame="world")`` / ``apply_torque(torque, frame="world")`` on a link item (applyExternalForce /
  applyExternalTorque; the reference's Item has no such method, Bullet does): dynamics mode: queued for the next ``world.step()``
  alone, which hands them (at most four) and any ``control_torque`` to the engine in one launch (``pnr_world_step_wrenches``) and
  clears them, as ``reset()`` does.  They act over the whole ``world.step()``; Bullet clears them after one stepSimulation
  (``PioneerVectorEnv.world_step(hold_substeps=1)``).  A fifth record and kinematic mode raise AssertionError.
* ``joint.state()`` / ``joint.acceleration()`` / ``scene.joint_states()``: pybullet.getJointState as ``JointState`` tuples (PyBullet's
  four field names), all six joints from ONE engine launch (``pnr_get_joint_states``).  Dynamics mode: what the first sub-step of the
  next ``world.step()`` would evaluate, looked at and not taken: the motor's torque after its cap, the reaction wrench the parent
  exerts on the joint's child link (Fx, Fy, Fz, Mx, My, Mz at the child link's origin, in its frame), and q̈.  Torques queued by
  ``control_torque`` and wrenches queued by ``apply_force`` / ``apply_torque`` are included and NOT consumed: the sensor sees the
  shove that is about to act.  Kinematic mode: position and velocity as ``position()`` / ``velocity()``; nothing is simulated there,
  so the reaction is six zeros, the torque 0.0 and the acceleration 0.0.  Sign and frame against Bullet's are unpinned.
* ``world.step()``: ``frame_skip`` × ``stepSimulation`` = ONE engine launch (``pnr_world_step``), nothing on the host.  Dynamics
  mode: the articulated-body sub-steps (gravity, contacts with the scene's bodies, limits, every joint's motor) and nothing else —
  no command integration, reward or observation.  Kinematic mode: each joint carries on at the velocity it was reset with
  (q += q̇ × step_time, stopped at its limit): what Bullet does without gravity, motor torque and collision shapes.
* links: ``scene.links`` / ``scene.links_by_name`` hold one item per URDF link, as load_scene makes one per joint
  (bullet_env.py:114-126), and ``joint.item`` is the joint's child link, as in the reference.  ``pose()`` / ``velocity()`` of a
  link are one engine launch each (``pnr_get_link_states``) for the one env: dynamics mode on the simulated joints; kinematic
  mode on the simulator's joints above (so after ``env.step`` every link's velocity is 0, and ``reset_state(p, v)`` gives the
  links downstream of that joint the velocity v moves them with, as in Bullet).  ``reset_pose`` on a link asserts, as the
  reference's does.  Deviation: link items are NOT in ``scene.items_by_name`` (which holds the created bodies and the target
  only); the reference's ``items_by_name['robot:pointer']`` is ``links_by_name['robot:pointer']`` here.
* ``render("rgb_array")`` with ``EngineConfig.renderer == "engine"`` draws every created body in ``scene.items`` (the target aside) in
  its ``Item.rgba_color``: the ``rgba_color`` it was created with, else the URDF's obstacle_mat; planes in ground_mat.
* ``scene.contact_points(item=None)`` / ``scene.closest_points(distance, item=None)``: pybullet.getContactPoints / getClosestPoints
  between the arm and the bodies created through ``env.scene`` with a collision shape, as ``ContactPoint`` tuples (PyBullet's field
  names), one engine launch (``pnr_get_contacts``), either mode.  The arm's geometry is the engine's 23 contact sample spheres
  (``CONTACT_SAMPLE_LINKS`` gives each one's URDF link): one entry per sample, against its nearest body.  bodyUniqueIdA is 0 (the
  arm), bodyUniqueIdB 1 + the body's place among the created collision bodies, linkIndexB -1 (a base).  Deviation: PyBullet's
  manifolds (several points per pair) are not reproduced.
* ``scene.path_clearance(waypoints, substeps=8, margin=0.0)``: no single PyBullet call — getClosestPoints at every interpolated
  configuration of the joint path ``waypoints`` against the created collision bodies, one engine launch (``pnr_path_clearance``),
  either mode, as a ``PathClearance`` (free, the smallest clearance, where on the path, the link and the body id that attain it, the
  first configuration under the margin).  A sampled check; ``path_substeps(waypoints, max_step)`` sizes ``substeps``.
* ``scene.ray_test(ray_from, ray_to)`` / ``scene.ray_test_batch(ray_froms, ray_tos, parent_item=None)``: pybullet.rayTest /
  rayTestBatch against the created collision bodies and the arm's visual shapes, as ``RayHit`` tuples (PyBullet's field names),
  one engine launch (``pnr_ray_test``), either mode; ``parent_item`` a link item in whose frame the rays are given.  Ids as in
  ``ContactPoint``: the arm is body 0 with linkIndex the URDF link, a created body 1 + its place among the created collision
  bodies with linkIndex -1; a miss is (-1, -1, 1.0, (0, 0, 0), (0, 0, 0)).  ``ray_fan(n, length, start)`` makes a range sensor's rays.
* ``Item.pose()`` is a ``Pose`` (``.xyz``, ``.rpy``), still a 2-tuple (position, orientation); ``Item.velocity()`` a ``Velocity``
  (linear, angular), zero for created bodies and the target (they are static).
Build-defined behaviour where the reference delegates to Bullet: parity unpinned, like the rest of the Bullet boundary.
"""
import dataclasses
import math
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _lib, model
from .config import SceneBody, scene_box, scene_plane, scene_sphere
from .render import GROUND_RGBA, OBSTACLE_RGBA


class Pose(NamedTuple):
    """bullet_scene.py:11-30: a world position and an orientation quaternion (x, y, z, w)."""
    position: Tuple[float, float, float]
    orientation: Tuple[float, float, float, float]

    @property
    def xyz(self) -> Tuple[float, float, float]:
        return self.position

    @property
    def rpy(self) -> Tuple[float, float, float]:
        return Scene.quat2rpy(self.orientation)


class Velocity(NamedTuple):
    """bullet_scene.py:33-36: world linear and angular velocity."""
    linear: Tuple[float, float, float]
    angular: Tuple[float, float, float]


class JointState(NamedTuple):
    """pybullet.getJointState, in PyBullet's names (the reference's binding decodes these four, bullet_bindings.py:48-51)."""
    joint_position: float
    joint_velocity: float
    joint_reaction_forces: Tuple[float, float, float, float, float, float]
    applied_joint_motor_torque: float


class ContactPoint(NamedTuple):
    """One entry of pybullet.getContactPoints / getClosestPoints, in PyBullet's names.  A is the arm, B the created body."""
    contactFlag: int
    bodyUniqueIdA: int
    bodyUniqueIdB: int
    linkIndexA: int
    linkIndexB: int
    positionOnA: Tuple[float, float, float]
    positionOnB: Tuple[float, float, float]
    contactNormalOnB: Tuple[float, float, float]
    contactDistance: float
    normalForce: float


class RayHit(NamedTuple):
    """One entry of pybullet.rayTest / rayTestBatch, in PyBullet's names.  A miss is (-1, -1, 1.0, (0, 0, 0), (0, 0, 0))."""
    objectUniqueId: int
    linkIndex: int
    hitFraction: float
    hitPosition: Tuple[float, float, float]
    hitNormal: Tuple[float, float, float]


class CameraImage(NamedTuple):
    """pybullet.getCameraImage's result, numpy arrays: rgb uint8 [height, width, 3], depth float32 [height, width] (the eye depth
    along the view axis, +inf where nothing is hit: not Bullet's depth buffer), seg uint8 [height, width] (``_lib.SEG_*``)."""
    width: int
    height: int
    rgb: np.ndarray
    depth: np.ndarray
    seg: np.ndarray


def ray_fan(n: int, length: float, start: float = 0.0) -> np.ndarray:
    """A range sensor's rays as a float32 ``[n, 6]`` array (from | to): ``n`` directions spread over the sphere (the Fibonacci
    lattice), each ray from ``start`` to ``length`` along its direction, in the frame the rays are cast in (for a sensor mounted
    on a link: ``ray_test(rays, parent_link=...)``).  ``start`` > 0 keeps the rays' origins off the mount's own surface."""
    k = np.arange(int(n), dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / float(n)
    r = np.sqrt(np.maximum(1.0 - z * z, 0.0))
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    d = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)
    return np.concatenate([float(start) * d, float(length) * d], axis=1).astype(np.float32)


def ik_start_table(S: int, seed: int = 0) -> np.ndarray:
    """The default starts of multi-start inverse kinematics (``PioneerVectorEnv.solve_ik_multi(starts=S)``) as a float32 ``[S, 6]``
    array: row 0 the rest pose q = 0, the others uniform in ±0.8 of the joint limits from ``np.random.default_rng(seed)``.  The
    draws go row by row, so the table of S starts is the first S rows of every larger table of the same seed."""
    limits = np.array([j.limit for j in model.revolute_joints()], dtype=np.float64)
    table = np.random.default_rng(int(seed)).uniform(-0.8, 0.8, size=(int(S), len(limits))) * limits
    table[0] = 0.0
    return table.astype(np.float32)


class IkPath(NamedTuple):
    """``PioneerKinematicEnv.solve_ik_path``'s answer for the one env: was every configuration of the pointer path reached, the
    first configuration that was not (-1: none), the joint path (float64 ``[C, 6]``; the rows after ``fail_at`` repeat that row), the
    largest distance and angle (rad) left over the configurations up to ``fail_at``, the joint travel sum |dq_j| over the path and
    the largest single joint move between two neighbouring configurations (a branch flip shows there)."""
    tracked: bool
    fail_at: int
    q_path: np.ndarray
    max_residual: float
    max_angle: float
    travel: float
    max_jump: float


class Trajectory(NamedTuple):
    """``PioneerKinematicEnv.retime_path``'s answer for the one env: do the limits admit the path at all, the time it takes (s; inf
    when not), the time at every row of the joint path (float64 ``[C]``) and the motor-target rows q | q̇ (float64 ``[steps, 12]``,
    one per world step; past the end they hold the last point, an infeasible path's hold the first)."""
    feasible: bool
    duration: float
    times: np.ndarray
    targets: np.ndarray


def steps_for(duration: float, dt: float) -> int:
    """How many samples at dt, 2 dt, .. cover a trajectory of ``duration``: the smallest count whose last sample is at or past the
    end, and so the trajectory's last point (at least 1).  A duration that is not finite (an infeasible path) gives 1."""
    if not (dt > 0):
        raise AssertionError(f"dt must be > 0, got {dt}")
    if not np.isfinite(duration) or duration <= 0:
        return 1
    return max(1, int(np.ceil(float(duration) / float(dt))))


class PathClearance(NamedTuple):
    """``Scene.path_clearance``'s answer for the one env: is the sampled path free, the smallest clearance on it, the path
    coordinate t where it is attained (segment index + fraction), the URDF link and the created body (``Scene.body_id``; 0 where
    there is no body) that attain it, and t of the first configuration with clearance < margin (-1.0: none)."""
    free: bool
    min_distance: float
    at: float
    link_name: str
    body_id: int
    first_hit: float


def path_substeps(waypoints, max_step: float) -> int:
    """The smallest ``substeps`` M of ``path_clearance`` for which no joint moves more than ``max_step`` rad between two
    neighbouring configurations of the path ``waypoints`` (``[K, 6]`` or ``[N, K, 6]``; a CPU tensor or anything numpy takes), at
    least 1.  On the host: the result sizes the launch.  More than 64 (``_lib.MAX_PATH_SUBSTEPS``) raises: add waypoints."""
    w = waypoints.detach().cpu().numpy() if isinstance(waypoints, torch.Tensor) else np.asarray(waypoints)
    w = w.astype(np.float64)
    if w.ndim not in (2, 3) or w.shape[-1] != 6:
        raise AssertionError(f"waypoints must have shape (K, 6) or (N, K, 6), got {w.shape}")
    if not max_step > 0:
        raise AssertionError("max_step must be > 0")
    if not np.isfinite(w).all():
        raise AssertionError("non-finite waypoints")
    longest = float(np.abs(np.diff(w, axis=-2)).max()) if w.shape[-2] > 1 else 0.0
    m = max(1, int(math.ceil(longest / float(max_step))))
    while m > 1 and longest / (m - 1) <= max_step:      # (ceil of a quotient that rounded up)
        m -= 1
    while longest / m > max_step:
        m += 1
    if m > _lib.MAX_PATH_SUBSTEPS:
        raise AssertionError(f"{m} sub-steps per segment exceed {_lib.MAX_PATH_SUBSTEPS}: add waypoints")
    return m


# the URDF link (Bullet's link_index) of each of the engine's 23 contact sample spheres, in the engine's order: 8 on arm1, 7 on
# arm2, 2 on rotator2 (+ hinge2), 3 on arm3, 2 on the effector's needle, and the pointer's own sphere
CONTACT_SAMPLE_LINKS = (3,) * 8 + (4,) * 7 + (5,) * 2 + (7,) * 3 + (9,) * 2 + (10,)
assert len(CONTACT_SAMPLE_LINKS) == _lib.CONTACT_SAMPLES

_ZERO3 = (0.0, 0.0, 0.0)


class Item:
    """bullet_scene.py:40-67's Item, for the bodies created through Scene (and the target marker)."""

    def __init__(self, name: Optional[str], shape: str, position, orientation, collision: bool, size, rgba_color=None):
        self.name, self.shape, self.collision, self.size = name, shape, bool(collision), tuple(size)
        self._position, self._orientation = tuple(map(float, position)), tuple(map(float, orientation))
        # the colour render("rgb_array") draws it in with EngineConfig.renderer == "engine"
        self.rgba_color = None if rgba_color is None else tuple(map(float, rgba_color))

    def pose(self) -> Pose:
        return Pose(self._position, self._orientation)

    def velocity(self) -> Velocity:
        return Velocity(_ZERO3, _ZERO3)                      # created bodies are static (mass 0), the target is a marker

    def __repr__(self) -> str:
        return f"Item(name={self.name}, shape={self.shape}, position={self._position}, collision={self.collision})"


class BodyItem(Item):
    """The scene's moving sphere (create_body_sphere with mass > 0): Item's base branch, getBasePositionAndOrientation /
    getBaseVelocity / resetBasePositionAndOrientation (bullet_scene.py:53-73), on the engine's sphere state.  A point mass with a
    radius: the orientation stays as created and the angular velocity is zero (rolling is not modelled)."""

    def __init__(self, scene: "Scene", name, radius, position, orientation, rgba_color):
        super().__init__(name, "sphere", position, orientation, True, (radius, 0.0, 0.0), rgba_color)
        self._scene = scene

    def _words(self) -> np.ndarray:
        return self._scene._env._vec.body_state()[0].double().cpu().numpy()

    def pose(self) -> Pose:
        return Pose(tuple(map(float, self._words()[0:3])), self._orientation)

    def velocity(self) -> Velocity:
        return Velocity(tuple(map(float, self._words()[3:6])), _ZERO3)

    def reset_pose(self, position, orientation):
        """resetBasePositionAndOrientation: the sphere at ``position``, at rest (Bullet zeroes the velocities too)"""
        self._orientation = tuple(map(float, orientation))
        self._scene._env._vec.set_body(position=tuple(map(float, position)), velocity=_ZERO3)


class LinkItem(Item):
    """A link item of load_scene (bullet_env.py:114-126): Item with a link_index, its pose and velocity from getLinkState
    (bullet_scene.py:53-67), here one pnr_get_link_states launch."""

    def __init__(self, scene: "Scene", name: str, link_index: int):
        super().__init__(name, "link", _ZERO3, (0.0, 0.0, 0.0, 1.0), False, ())
        self._scene, self.link_index = scene, link_index

    def _record(self) -> np.ndarray:
        vec = self._scene._env._vec
        js = None if vec.engine_config.mode == "dynamic" else self._scene._bullet
        return vec.link_states(js)[0, self.link_index].double().cpu().numpy()

    def pose(self) -> Pose:
        r = self._record()
        return Pose(tuple(map(float, r[0:3])), tuple(map(float, r[3:7])))

    def velocity(self) -> Velocity:
        r = self._record()
        return Velocity(tuple(map(float, r[7:10])), tuple(map(float, r[10:13])))

    def reset_pose(self, position, orientation):
        raise AssertionError("Position can be reset only for base items: to control linked items use joint methods")   # :69-71

    def camera_image(self, width: int, height: int, position=_ZERO3, orientation=(0.0, 0.0, 0.0, 1.0), fov: float = 60.0,
                     near: float = 0.05, far: float = 200.0) -> "CameraImage":
        """getCameraImage from a camera mounted on this link (the view matrix from getLinkState, bullet_scene.py:53-59): the camera
        frame (x right, y up, looking along -z) sits at ``position`` / ``orientation`` (quaternion x, y, z, w) of the link's frame.
        One engine launch (``PioneerVectorEnv.render_frames(camera_link=..., cameras=...)``) drawing the arm, the target and the
        scene's ``render_bodies()``, on the joints ``render("rgb_array")`` draws: dynamics mode the simulated ones, kinematic
        mode the simulator's.  ``depth`` is the eye depth along the view axis (+inf where nothing is hit), not Bullet's depth
        buffer; ``seg`` holds the engine's labels (``_lib.SEG_*``).  Keep the camera outside the link's own shapes: from inside
        one it sees that shape's far face."""
        from .config import RenderConfig
        scene = self._scene
        vec = scene._env._vec
        bodies = scene.render_bodies()
        if len(bodies) > _lib.MAX_SCENE:
            raise AssertionError(f"the engine renderer draws at most {_lib.MAX_SCENE} created bodies, the scene has {len(bodies)}")
        cfg = RenderConfig(render_width=int(width), render_height=int(height), projection_fov=float(fov), projection_near=float(near),
                           projection_far=float(far))
        js = None if vec.engine_config.mode == "dynamic" else scene._bullet
        cam = np.asarray(tuple(position) + tuple(orientation), dtype=np.float32)
        fr = vec.render_frames(cfg, joint_state=js, bodies=bodies, depth=True, segmentation=True, camera_link=self.link_index, cameras=cam)
        return CameraImage(int(width), int(height), *(fr[k][0].cpu().numpy() for k in ("rgb", "depth", "seg")))

    def _queue_wrench(self, what: str, frame: str, force, position, torque):
        env = self._scene._env
        assert env._vec.engine_config.mode == "dynamic", f"{what}: external forces exist in dynamics mode only"
        assert frame in ("link", "world"), f"{what}: frame must be 'link' or 'world', got {frame!r}"
        queue = env.world._wrenches
        assert len(queue) < _lib.MAX_LINK_WRENCHES, f"{what}: at most {_lib.MAX_LINK_WRENCHES} forces and torques per world.step()"
        if position is None:                                                   # the link origin, in the record's frame
            position = self.pose().position if frame == "world" else _ZERO3
        queue.append(((self.link_index, frame), tuple(map(float, force)) + tuple(map(float, position)) + tuple(map(float, torque))))

    def apply_force(self, force, position=None, frame: str = "world"):
        """applyExternalForce on this link for the NEXT ``world.step()`` only (``pnr_world_step_wrenches``; the step consumes the
        queued forces and torques, at most four, and clears them).  ``frame`` ``"world"``: a world force at the world point
        ``position``, taken on the link at the step's first pose; ``"link"``: a force that turns with the link, at a point of the
        link's frame.  ``position=None``: the link origin.  Dynamics mode only."""
        self._queue_wrench("apply_force", frame, force, position, _ZERO3)

    def apply_torque(self, torque, frame: str = "world"):
        """applyExternalTorque on this link for the NEXT ``world.step()`` only; see ``apply_force``."""
        self._queue_wrench("apply_torque", frame, _ZERO3, _ZERO3, torque)

    def __repr__(self) -> str:
        return f"Item(name={self.name}, link_index={self.link_index})"


class Joint:
    def __init__(self, env, index: int, jd: model.JointDef):
        self._env, self.index, self.name = env, index, jd.name
        self.item: Optional[Item] = None                                       # the child link, set by Scene
        self.joint_type = jd.type
        lo, hi = env.joint_limits()
        self.lower_limit, self.upper_limit = float(lo[index]), float(hi[index])      # the float32 limits the env uses (:56)
        self.max_force = model.EFFORT
        self.damping = self.friction = 0.0

    def __repr__(self) -> str:
        return f"Joint(name={self.name}, index={self.index}, lower_limit={self.lower_limit}, upper_limit={self.upper_limit})"

    def _dynamic(self) -> bool:
        return self._env._vec.engine_config.mode == "dynamic"

    def position(self) -> float:
        if self._dynamic():
            return float(self._env._vec.get_dyn_state()[self.index, 0])
        return float(self._env.scene._bullet[0, self.index])

    def velocity(self) -> float:
        if self._dynamic():
            return float(self._env._vec.get_dyn_state()[6 + self.index, 0])
        return float(self._env.scene._bullet[0, 6 + self.index])

    def state(self) -> JointState:
        """getJointState of this joint (module docstring).  Every call is one engine launch and a copy to the host, and that
        launch answers all six joints: to read several, call ``Scene.joint_states()`` once."""
        return self._env.scene.joint_states()[self.index]

    def acceleration(self) -> float:
        """q̈ the next ``world.step()``'s first sub-step would integrate (before its joint-limit clamp); 0.0 in kinematic mode.
        One launch and host copy per call, as ``state()``."""
        return float(self._env.scene._joint_state_tensors()[0][self.index, 2])

    def reset_state(self, position: float, velocity: Optional[float] = None):
        """resetJointState (bullet_scene.py:157-165): the SIMULATOR's joint is put at ``position`` (and ``velocity``, else 0); the
        env's own r / v are not touched (the reference's are not either)."""
        v = 0.0 if velocity is None else float(velocity)
        if self._dynamic():
            vec = self._env._vec
            d = vec.get_dyn_state()
            d[self.index, 0] = float(position)
            d[6 + self.index, 0] = v
            vec.set_dyn_state(d)
        else:
            b = self._env.scene._bullet
            b[0, self.index] = float(position)
            b[0, 6 + self.index] = v

    def _set_motor(self, mode, position, velocity, position_gain, velocity_gain, max_force, max_velocity):
        nan = float("nan")
        args = (self.index, mode, nan if position is None else float(position), nan if velocity is None else float(velocity),
                nan if position_gain is None else float(position_gain), nan if velocity_gain is None else float(velocity_gain),
                nan if max_force is None else float(max_force), nan if max_velocity is None else float(max_velocity))
        self._env._vec.set_joint_motor(*args)
        self._env._motor_cmds[self.index] = args                  # re-applied when the engine handle is rebuilt (a body created later)

    def _constraint(self) -> bool:
        return self._env._vec.engine_config.joint_motor == "constraint"

    def control_position(self, position: float, velocity: Optional[float] = None, max_velocity: Optional[float] = None,
                         max_force: Optional[float] = None, position_gain: Optional[float] = None, velocity_gain: Optional[float] = None):
        """setJointMotorControl2(POSITION_CONTROL, ...) (bullet_scene.py:123-142) for ``world.step()``."""
        mode = _lib.CONTROL_POSITION_CONSTRAINT if self._constraint() else _lib.CONTROL_POSITION
        self._set_motor(mode, position, velocity, position_gain, velocity_gain, max_force, max_velocity)

    def control_velocity(self, velocity: float, max_force: Optional[float] = None):
        """setJointMotorControl2(VELOCITY_CONTROL, ...) (bullet_scene.py:144-155) for ``world.step()``."""
        mode = _lib.CONTROL_VELOCITY_CONSTRAINT if self._constraint() else _lib.CONTROL_VELOCITY
        self._set_motor(mode, None, velocity, None, None, max_force, None)

    def control_torque(self, torque: float):
        """setJointMotorControl2(TORQUE_CONTROL, force=torque): this joint's torque for the NEXT ``world.step()`` only (the step
        applies the recorded torques through ``world_step(joint_torques=...)`` and clears them).  It is added to what the joint's
        motor gives, so pure torque control first gives the joint zero gains on the engine's PD law
        (``vec.set_joint_motor(j, CONTROL_VELOCITY, target_velocity=0, velocity_gain=0)``), as one disables Bullet's default
        motor.  Dynamics mode with the PD motors only."""
        if not self._dynamic():
            raise _lib.PnrError(-5, "Joint.control_torque: joint torques exist in dynamics mode only")
        if self._constraint():
            raise _lib.PnrError(-5, "Joint.control_torque: not built together with joint_motor=\"constraint\" (the boxed solve)")
        self._env.world._torques[self.index] = float(torque)


class Scene:
    def __init__(self, env):
        self._env = env
        self.items: List[Item] = []
        self.items_by_name: Dict[str, Item] = {}
        # one item per URDF link (Bullet's link_index order); kept out of items_by_name (module docstring)
        self.links: List[LinkItem] = [LinkItem(self, name, k) for k, name in enumerate(model.LINK_NAMES)]
        self.links_by_name: Dict[str, LinkItem] = {li.name: li for li in self.links}
        self.joints: List[Joint] = [Joint(env, i, jd) for i, jd in enumerate(model.revolute_joints())]
        self.joints_by_name: Dict[str, Joint] = {j.name: j for j in self.joints}
        for j, jd in zip(self.joints, model.revolute_joints()):
            j.item = self.links_by_name[jd.child]                              # the joint's child link (bullet_env.py:120-126)
        # kinematic mode: the simulator's joints (q | qd) as act() leaves them in Bullet; see the module docstring
        self._bullet = torch.zeros((1, 12), dtype=torch.float32, device=env._vec.device)
        self._grip: Optional[int] = None                                       # create_constraint's id while the grip exists

    def sync_from_env(self):
        """What act() does to the Bullet client on every step (pioneer_knm_env.py:148): joints at the env's r, velocity 0."""
        if self._env._vec.engine_config.mode != "dynamic":
            self._bullet[0, 0:6] = self._env._vec.get_state().view(torch.float32)[12:18, 0]
            self._bullet[0, 6:12] = 0.0

    def _joint_state_tensors(self):
        """(joints [6, 4] = q, q̇, q̈, τ_motor; reaction [6, 6]) of the one env as host arrays, from one launch; kinematic mode: the
        simulator's q, q̇ and zeros."""
        vec = self._env._vec
        if vec.engine_config.mode != "dynamic":
            joints = np.zeros((6, 4))
            joints[:, 0:2] = self._bullet[0].cpu().numpy().reshape(2, 6).T
            return joints, np.zeros((6, 6))
        world = self._env.world
        tau = world._torque_tensor(vec.device) if world._torques else None
        wr = world._wrench_records(vec.device) if world._wrenches else None
        res = vec.joint_states(joint_torques=tau, link_wrenches=wr)
        return res["joints"][0].cpu().numpy(), res["reaction"][0].cpu().numpy()

    def joint_states(self) -> List[JointState]:
        """getJointStates of the six joints, one engine launch (module docstring): what is queued for the next ``world.step()`` is
        included and stays queued."""
        joints, reaction = self._joint_state_tensors()
        return [JointState(float(joints[i, 0]), float(joints[i, 1]), tuple(float(x) for x in reaction[i]), float(joints[i, 3]))
                for i in range(6)]

    # -- items -----------------------------------------------------------------------------------------------------------
    def add_item(self, item: Item):
        self.items.append(item)
        if item.name is not None:
            assert item.name not in self.items_by_name                        # bullet_scene.py:181-183
            self.items_by_name[item.name] = item

    def _create(self, item: Item, mass: float, body):
        assert float(mass) == 0.0, "only static bodies (mass 0) and one moving sphere are modelled: the reference never creates a moving one"
        self.add_item(item)
        vec = self._env._vec
        if item.collision and vec.engine_config.mode == "dynamic":
            self._env._rebuild_engine(dataclasses.replace(vec.engine_config, scene=tuple(vec.engine_config.scene) + (body,)))

    def create_body_sphere(self, name, collision, mass, radius, position, orientation, rgba_color=None):   # bullet_scene.py:193-204
        if float(mass) > 0.0:                                                  # the engine's one moving sphere (module docstring)
            vec = self._env._vec
            assert vec.engine_config.mode == "dynamic", "a moving sphere (mass > 0) exists in dynamics mode only"
            assert collision, "a moving sphere without a collision shape is not modelled"
            assert not any(isinstance(i, BodyItem) for i in self.items), "the engine models one moving sphere per env: there is one already"
            self.add_item(BodyItem(self, name, float(radius), position, orientation, rgba_color or OBSTACLE_RGBA))
            vec.set_body(mass=float(mass), radius=float(radius), position=tuple(map(float, position)), velocity=_ZERO3)
            vec.set_body_queries(rays=True, contacts=True)                     # (render_bodies draws it: not a second time)
            return
        self._create(Item(name, "sphere", position, orientation, collision, (radius, 0.0, 0.0), rgba_color or OBSTACLE_RGBA), mass,
                     scene_sphere(radius, position, orientation))

    def create_body_box(self, name, collision, mass, half_extents, position, orientation, rgba_color=None):  # :206-217
        self._create(Item(name, "box", position, orientation, collision, half_extents, rgba_color or OBSTACLE_RGBA), mass,
                     scene_box(half_extents, position, orientation))

    def create_body_plane(self, name, mass, normal, position, orientation):                                   # :219-227
        self._create(Item(name, "plane", position, orientation, True, normal, GROUND_RGBA), mass, scene_plane(normal, position, orientation))

    # -- the grip (pybullet.createConstraint JOINT_POINT2POINT / changeConstraint / removeConstraint / getConstraintState) ----
    _GRIP_ID = 1                                                               # the one constraint's userConstraintUniqueId

    def create_constraint(self, parent, child, max_force: float, anchor=None, direction=None) -> int:
        """createConstraint(arm, pointerLink, body, -1, JOINT_POINT2POINT, ...) + changeConstraint(maxForce): the moving sphere
        held at a point of ``robot:pointer`` (``PioneerVectorEnv.set_body_grip``; a suction or magnet gripper).  ``parent`` is
        ``links_by_name["robot:pointer"]`` and ``child`` the created moving sphere: nothing else is modelled.  ``anchor`` /
        ``direction``: the grip's params (None: the defaults, the sphere tangent to the pointer's own sphere)."""
        assert parent is self.links_by_name["robot:pointer"], "the grip is modelled on link robot:pointer only"
        assert isinstance(child, BodyItem) and child is self.moving_body(), "the grip holds the created moving sphere (create_body_sphere with mass > 0) only"
        assert self._grip is None, "the engine models one grip per env: there is one already"
        assert float(max_force) > 0.0, "a constraint with max_force <= 0 holds nothing"
        params = {k: tuple(map(float, v)) for k, v in (("anchor", anchor), ("direction", direction)) if v is not None}
        self._env._vec.set_body_grip(params, max_force=float(max_force))
        self._grip = self._GRIP_ID
        return self._grip

    def _check_constraint(self, constraint_id: int):
        assert self._grip is not None and constraint_id == self._grip, f"no such constraint: {constraint_id}"

    def remove_constraint(self, constraint_id: int):
        """removeConstraint: the sphere is released (max_force 0) and follows the sphere's own law again, arm contacts included."""
        self._check_constraint(constraint_id)
        self._env._vec.set_body_grip(max_force=0.0)
        self._grip = None

    def change_constraint(self, constraint_id: int, max_force: float):
        """changeConstraint(maxForce)"""
        self._check_constraint(constraint_id)
        assert float(max_force) > 0.0, "a constraint with max_force <= 0 holds nothing: remove_constraint releases"
        self._env._vec.set_body_grip(max_force=float(max_force))

    def constraint_state(self, constraint_id: int) -> Tuple[float, float, float]:
        """getConstraintState: the world-frame force on the sphere in the last sub-step of the last ``world.step()``"""
        self._check_constraint(constraint_id)
        return tuple(map(float, self._env._vec.body_grip()[0, 1:4].double().cpu().numpy()))

    def render_bodies(self):
        """The created bodies as render_frames draws them: (SceneBody, rgba) of every item but the target."""
        return [(SceneBody(i.shape, i.pose().position, i._orientation, tuple(map(float, i.size))), i.rgba_color or OBSTACLE_RGBA)
                for i in self.items if i.name != "target"]           # (the moving sphere where it is now)

    # -- contacts (pybullet.getContactPoints / getClosestPoints) ------------------------------------------------------------
    def collision_items(self) -> List[Item]:
        """The created bodies with a collision shape, in creation order: a body's place here is its body index in the engine's
        query and bodyUniqueIdB - 1."""
        return [i for i in self.items if i.collision and i.name != "target" and not isinstance(i, (LinkItem, BodyItem))]

    def moving_body(self) -> Optional["BodyItem"]:
        """The scene's moving sphere, if one was created."""
        return next((i for i in self.items if isinstance(i, BodyItem)), None)

    def body_id(self, item: Item) -> int:
        """bodyUniqueIdB / objectUniqueId of a created collision body: 1 + its place in ``collision_items()``; the moving sphere's
        is one past the last of them (the engine reports it after the static bodies)."""
        bodies = self.collision_items()
        return 1 + (len(bodies) if isinstance(item, BodyItem) else bodies.index(item))

    def _contact_records(self, item: Optional[Item], keep) -> List[ContactPoint]:
        bodies = self.collision_items()
        if len(bodies) > _lib.MAX_SCENE:
            raise AssertionError(f"the engine queries at most {_lib.MAX_SCENE} created bodies, the scene has {len(bodies)}")
        vec = self._env._vec
        js = None if vec.engine_config.mode == "dynamic" else self._bullet
        sb = [SceneBody(i.shape, i._position, i._orientation, tuple(map(float, i.size))) for i in bodies]
        rec = vec.contacts(joint_state=js, bodies=sb, summary=False)["points"][0].double().cpu().numpy()
        out = []
        for s, r in enumerate(rec):
            b = int(r[7])
            if b < 0 or not keep(float(r[0])):
                continue
            if isinstance(item, LinkItem) and CONTACT_SAMPLE_LINKS[s] != item.link_index:
                continue
            hit = self.moving_body() if b == _lib.MAX_SCENE else bodies[b]   # (body MAX_SCENE: the moving sphere)
            if item is not None and not isinstance(item, LinkItem) and hit is not item:
                continue
            n, on_a = r[1:4], r[4:7]
            out.append(ContactPoint(0, 0, self.body_id(hit), CONTACT_SAMPLE_LINKS[s], -1, tuple(map(float, on_a)), tuple(map(float, on_a - r[0] * n)),
                                    tuple(map(float, n)), float(r[0]), float(r[8])))
        return out

    def contact_points(self, item: Optional[Item] = None) -> List[ContactPoint]:
        """getContactPoints: the samples that penetrate their nearest created body (contactDistance < 0).  ``item``: a link item
        (only that link's samples) or a created body (only contacts with it)."""
        return self._contact_records(item, lambda d: d < 0.0)

    def closest_points(self, distance: float, item: Optional[Item] = None) -> List[ContactPoint]:
        """getClosestPoints: the samples within ``distance`` of their nearest created body (contactDistance <= distance)."""
        return self._contact_records(item, lambda d: d <= float(distance))

    def path_clearance(self, waypoints, substeps: int = 8, margin: float = 0.0) -> PathClearance:
        """Sweeps the arm along the joint path ``waypoints`` (``[K, 6]``) against the created collision bodies (and the moving
        sphere where it stands), ``substeps`` configurations per segment, one engine launch (``PioneerVectorEnv.path_clearance``:
        a sampled check).  Body ids as in ``contact_points``."""
        bodies = self.collision_items()
        if len(bodies) > _lib.MAX_SCENE:
            raise AssertionError(f"the engine queries at most {_lib.MAX_SCENE} created bodies, the scene has {len(bodies)}")
        sb = [SceneBody(i.shape, i._position, i._orientation, tuple(map(float, i.size))) for i in bodies]
        wp = torch.as_tensor(np.asarray(waypoints, dtype=np.float32)).reshape(-1, 6)
        sm = self._env._vec.path_clearance(wp, substeps=substeps, bodies=sb, margin=margin)["summary"][0].double().cpu().numpy()
        b = int(sm[3])
        hit = None if b < 0 else (self.moving_body() if b == _lib.MAX_SCENE else bodies[b])
        return PathClearance(bool(sm[6] > 0), float(sm[0]), float(sm[1]), model.LINK_NAMES[CONTACT_SAMPLE_LINKS[int(sm[2])]],
                             0 if hit is None else self.body_id(hit), float(sm[4]))

    # -- ray casts (pybullet.rayTest / rayTestBatch) ---------------------------------------------------------------------------
    @staticmethod
    def _ray_hits(hits: np.ndarray, moving_id: int = -1) -> List[RayHit]:
        """pnr_ray_test's ``[R, 8]`` rows as RayHit tuples: the arm is body 0 with linkIndex the URDF link, a created body
        1 + its place in ``collision_items()`` with linkIndex -1 (the moving sphere: ``moving_id``, its item's ``body_id``), a miss PyBullet's
        (-1, -1, 1.0, (0, 0, 0), (0, 0, 0))."""
        out = []
        for r in np.asarray(hits, dtype=np.float64):
            label = int(r[7])
            if label == _lib.SEG_BACKGROUND or label == _lib.SEG_TARGET:       # (the façade never enables the target)
                out.append(RayHit(-1, -1, 1.0, _ZERO3, _ZERO3))
                continue
            if label == _lib.SEG_MOVING_BODY:
                body, link = moving_id, -1
            else:
                body, link = (1 + label - _lib.SEG_BODY0, -1) if label >= _lib.SEG_BODY0 else (0, label - _lib.SEG_LINK0)
            out.append(RayHit(body, link, float(r[0]), tuple(map(float, r[1:4])), tuple(map(float, r[4:7]))))
        return out

    def ray_test_batch(self, ray_froms, ray_tos, parent_item: Optional[LinkItem] = None) -> List[RayHit]:
        """rayTestBatch: one RayHit per ray against the bodies created through ``env.scene`` with a collision shape and the arm's
        visual shapes, one engine launch (``pnr_ray_test``), either mode.  ``parent_item``: a link item (``links_by_name[...]``)
        in whose frame the rays are given (PyBullet's parentObjectUniqueId / parentLinkIndex); None: the world frame.  Deviation:
        Bullet casts against collision shapes, of which the reference's arm has none; here the arm is its visual shapes."""
        bodies = self.collision_items()
        if len(bodies) > _lib.MAX_SCENE:
            raise AssertionError(f"the engine queries at most {_lib.MAX_SCENE} created bodies, the scene has {len(bodies)}")
        if parent_item is not None and not isinstance(parent_item, LinkItem):
            raise AssertionError("parent_item must be a link item (scene.links_by_name[...])")
        rays = np.concatenate([np.asarray(ray_froms, dtype=np.float32).reshape(-1, 3), np.asarray(ray_tos, dtype=np.float32).reshape(-1, 3)], axis=1)
        vec = self._env._vec
        js = None if vec.engine_config.mode == "dynamic" else self._bullet
        sb = [SceneBody(i.shape, i._position, i._orientation, tuple(map(float, i.size))) for i in bodies]
        hits = vec.ray_test(rays, parent_link=-1 if parent_item is None else parent_item.link_index, hit_arm=True, bodies=sb,
                            joint_state=js)["hits"][0].cpu().numpy()
        sphere = self.moving_body()
        return self._ray_hits(hits, -1 if sphere is None else self.body_id(sphere))

    def ray_test(self, ray_from, ray_to) -> RayHit:
        """rayTest: the first hit of the segment ray_from -> ray_to (world frame); see ``ray_test_batch``."""
        return self.ray_test_batch([ray_from], [ray_to])[0]

    # -- rotations (pybullet.getQuaternionFromEuler / getEulerFromQuaternion: x, y, z, w; roll about x, pitch about y, yaw about z) --
    @staticmethod
    def rpy2quat(rpy: Tuple[float, float, float]):
        r, p, y = (0.5 * float(a) for a in rpy)
        cr, sr, cp, sp, cy, sy = math.cos(r), math.sin(r), math.cos(p), math.sin(p), math.cos(y), math.sin(y)
        return (sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy)

    @staticmethod
    def quat2rpy(quat: Tuple[float, float, float, float]):
        x, y, z, w = (float(a) for a in quat)
        roll = math.atan2(2.0 * (w * x + y * z), 1.0 - 2.0 * (x * x + y * y))
        pitch = math.asin(max(-1.0, min(1.0, 2.0 * (w * y - z * x))))
        yaw = math.atan2(2.0 * (w * z + x * y), 1.0 - 2.0 * (y * y + z * z))
        return (roll, pitch, yaw)

    def __repr__(self) -> str:
        items_str = "\n".join(f"\t\t{x}" for x in self.items)
        joints_str = "\n".join(f"\t\t{x}" for x in self.joints)
        return f"Scene(\n\titems: \n{items_str} \n\tjoints: \n{joints_str} \n)"


class World:
    """bullet_scene.py:262-279."""

    def __init__(self, env):
        self._env = env
        sc = env.simulation_config
        self.timestep, self.frame_skip, self.gravity_force = sc.timestep, sc.frame_skip, sc.gravity
        self._torques: Dict[int, float] = {}                                   # Joint.control_torque: joint -> torque of the next step
        self._wrenches: List[tuple] = []                                       # LinkItem.apply_force / apply_torque: ((link, frame), 9 floats)

    @property
    def step_time(self) -> float:
        return self.timestep * self.frame_skip

    def _torque_tensor(self, device):
        """the queued ``control_torque`` values as the engine's [1, 6] tensor"""
        return torch.tensor([[self._torques.get(j, 0.0) for j in range(6)]], dtype=torch.float32, device=device)

    def _wrench_records(self, device):
        """the queued ``apply_force`` / ``apply_torque`` records as ``world_step``'s ``(specs, [1, K, 9] tensor)``"""
        return [s for s, _ in self._wrenches], torch.tensor([[w for _, w in self._wrenches]], dtype=torch.float32, device=device)

    def step(self):
        """frame_skip x stepSimulation: ONE launch of the engine (pnr_world_step), no host arithmetic."""
        vec = self._env._vec
        tau = None
        if self._torques:                                                      # recorded for this step alone (TORQUE_CONTROL)
            tau = self._torque_tensor(vec.device)
            self._torques = {}
        if self._wrenches:                                                     # .. and the links' external forces and torques
            specs, rec = self._wrench_records(vec.device)
            self._wrenches = []
            vec.world_step(joint_torques=tau, link_wrenches=(specs, rec))
            return
        if tau is not None:
            vec.world_step(joint_torques=tau)
            return
        vec.world_step(None if vec.engine_config.mode == "dynamic" else self._env.scene._bullet)
