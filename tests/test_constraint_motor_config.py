"""CPU checks of Bullet's constraint motor surface (no GPU): EngineConfig.joint_motor, the _lib constants against the header's
enum pnr_control, Bullet's recalled defaults in the header, and which control mode the facade's Joint.control_position /
control_velocity send under each EngineConfig.joint_motor."""
import math
import re

import numpy as np
import pytest

from pioneer_amd import EngineConfig, _lib, model
from pioneer_amd.scene import Joint


def _header():
    with open(_lib.HEADER) as f:
        return f.read()


def test_joint_motor_defaults_to_pd_and_rejects_other_values():
    assert EngineConfig().joint_motor == "pd"
    assert EngineConfig(joint_motor="constraint").joint_motor == "constraint"
    for bad in ("bullet", "PD", "", None):
        with pytest.raises(ValueError):
            EngineConfig(joint_motor=bad)
    import dataclasses
    with pytest.raises(ValueError):
        dataclasses.replace(EngineConfig(), joint_motor="velocity")


def test_lib_constants_equal_the_header_enum():
    """Parsed from include/pioneer_amd.h the way _lib._header_abi_version reads PNR_ABI_VERSION."""
    src = _header()
    body = re.search(r"enum\s+pnr_control\s*\{(.*?)\};", src, re.S).group(1)
    values = {m.group(1): int(m.group(2)) for m in re.finditer(r"PNR_CONTROL_(\w+)\s*=\s*(\d+)", body)}
    assert values == {"POSITION": _lib.CONTROL_POSITION, "VELOCITY": _lib.CONTROL_VELOCITY,
                      "POSITION_CONSTRAINT": _lib.CONTROL_POSITION_CONSTRAINT,
                      "VELOCITY_CONSTRAINT": _lib.CONTROL_VELOCITY_CONSTRAINT}
    assert (_lib.CONTROL_POSITION_CONSTRAINT, _lib.CONTROL_VELOCITY_CONSTRAINT) == (2, 3)
    assert _lib.ABI_VERSION == 5                                       # additive: the ABI version stays


def test_bullet_defaults_are_stated_once_in_the_header():
    src = _header()
    got = {m.group(1): float(m.group(2)) for m in re.finditer(r"^#define\s+PNR_BULLET_(\w+)\s+([-+0-9.eE]+)", src, re.M)}
    assert got == {"POSITION_GAIN": 0.1, "VELOCITY_GAIN": 1.0, "TARGET_VELOCITY": 0.0, "MAX_FORCE": 100000.0, "MAX_VELOCITY": 0.0}
    for line in re.findall(r"^#define\s+PNR_BULLET_\w+.*$", src, re.M):
        assert "recalled" in line and "not verified" in line, line


def test_joint_motor_is_not_part_of_pnr_config():
    """Python-side only: the C struct is the same bytes for both laws."""
    from pioneer_amd import PioneerKinematicConfig, SimulationConfig
    from pioneer_amd.config import to_c_config
    a = to_c_config(PioneerKinematicConfig(), SimulationConfig(), EngineConfig(mode="dynamic"))
    b = to_c_config(PioneerKinematicConfig(), SimulationConfig(), EngineConfig(mode="dynamic", joint_motor="constraint"))
    assert bytes(a) == bytes(b)


class _Vec:
    def __init__(self, joint_motor):
        self.engine_config = EngineConfig(mode="dynamic", joint_motor=joint_motor)
        self.calls = []

    def set_joint_motor(self, *args):
        self.calls.append(args)


class _Env:
    def __init__(self, joint_motor):
        self._vec = _Vec(joint_motor)
        self._motor_cmds = {}

    def joint_limits(self):
        return -np.ones(_lib.DOF, np.float32), np.ones(_lib.DOF, np.float32)


def _joint(joint_motor, index=2):
    env = _Env(joint_motor)
    return env, Joint(env, index, model.revolute_joints()[index])


def _same(a, b):
    return len(a) == len(b) and all((isinstance(x, float) and math.isnan(x) and math.isnan(y)) or x == y for x, y in zip(a, b))


def test_facade_sends_the_constraint_modes_with_omitted_arguments_left_to_the_engine():
    nan = float("nan")
    env, j = _joint("constraint")
    j.control_velocity(0.8)
    j.control_velocity(0.0, max_force=0)
    j.control_position(0.5)
    j.control_position(0.5, velocity=0.1, max_velocity=0.3, max_force=7.0, position_gain=0.2, velocity_gain=0.9)
    want = [(2, _lib.CONTROL_VELOCITY_CONSTRAINT, nan, 0.8, nan, nan, nan, nan),
            (2, _lib.CONTROL_VELOCITY_CONSTRAINT, nan, 0.0, nan, nan, 0.0, nan),
            (2, _lib.CONTROL_POSITION_CONSTRAINT, 0.5, nan, nan, nan, nan, nan),
            (2, _lib.CONTROL_POSITION_CONSTRAINT, 0.5, 0.1, 0.2, 0.9, 7.0, 0.3)]
    assert len(env._vec.calls) == len(want)
    for got, w in zip(env._vec.calls, want):
        assert _same(got, w), (got, w)
    assert _same(env._motor_cmds[2], want[-1])                        # what a rebuilt handle re-applies


def test_facade_on_pd_sends_the_pd_modes_as_before():
    nan = float("nan")
    env, j = _joint("pd", index=0)
    j.control_velocity(0.8, max_force=900)
    j.control_position(-0.5)
    assert _same(env._vec.calls[0], (0, _lib.CONTROL_VELOCITY, nan, 0.8, nan, nan, 900.0, nan))
    assert _same(env._vec.calls[1], (0, _lib.CONTROL_POSITION, -0.5, nan, nan, nan, nan, nan))
