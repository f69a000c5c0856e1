"""Building the float64 oracle of a test case, stated once for the *_cases.py files, which keep their case tables and call these.
Nothing here is a reference or an input set.
"""
import numpy as np

from oracle import DynOracle
from oracle.binding import ORC_DEV

DOF = 6
ORACLE_NAMES = dict(pd_kp="kp", pd_kd="kd")                           # every other EngineConfig argument has the oracle's name


def oracle_dyn(engine, gravity):
    """The oracle's params for EngineConfig arguments: the inverse of gpu_support.engine_config_from_oracle_names (whatever is
    left out takes the value both sides default to)."""
    return dict({ORACLE_NAMES.get(k, k): int(v) if isinstance(v, bool) else v for k, v in engine.items()}, gravity=gravity)


def command_actions(seed, steps, n, a_max):
    """the actions of the vector steps that move the command state off its reset values before the motors are set"""
    rng = np.random.default_rng(1000 + seed)
    return [(rng.uniform(-0.3, 0.3, (n, DOF)) * a_max).astype(np.float32) for _ in range(steps)]


def make_oracle(seed, n, frame_skip, gravity, engine, command_steps=0, reset=True):
    """The float64 oracle of a case after its reset and command steps: per-env link scales, friction, damping and command state as
    the engine draws them from the same seed (tests/test_gpu_dynamics.py holds the two to the same bits)."""
    orc = DynOracle(n, seed=seed, precision=ORC_DEV, frame_skip=frame_skip, dyn=oracle_dyn(engine, gravity))
    if reset:
        orc.reset(want_obs=False)
        for act in command_actions(seed, command_steps, n, orc.a_max):
            orc.step(act, want_obs=False)
    return orc


def load_states(orc, q, qd, scales=None, friction=None, damping=None):
    """Put q, qd [n, 6] (and optionally the per-env parameters) into the oracle's dynamics state."""
    orc.dstate["q"], orc.dstate["qd"] = np.asarray(q, dtype=np.float64), np.asarray(qd, dtype=np.float64)
    for name, v in (("mass_scale", scales), ("friction", friction), ("damping", damping)):
        if v is not None:
            orc.dstate[name] = np.asarray(v, dtype=np.float64)
