"""The joints a handle holds, read back from its raw state: what the GPU query tests compare the engine's results against."""
import torch


def kin_joints(env):
    """(q, qd) float32 [N, 6] of a kinematic-mode env: r (state words 12-17) and v (6-11)"""
    f = env.get_state().view(torch.float32).cpu().numpy()
    return f[12:18].T.copy(), f[6:12].T.copy()


def dyn_joints(env):
    """(q, qd) float32 [N, 6] of a dynamics-mode env: dyn words 0-5 and 6-11"""
    d = env.get_dyn_state().cpu().numpy()
    return d[0:6].T.copy(), d[6:12].T.copy()
