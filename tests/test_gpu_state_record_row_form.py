"""The state record's hot and cold parts (pnr_device.h) in the row-pass form of step_kernel against the form without the row
pass: `n` envs stepped as one handle (32 768 < n <= 65 536: the row pass) and the same envs, by global id, stepped as two handles
of at most 32 768 (the one-pass form with obs_tile_out) give the same bits — the comparison
tests/test_gpu_parity.py::test_split_batch_on_two_streams_equals_one_launch_bit_for_bit makes for 65 536.

Two steps with max_episode_steps = 2: the first with `info` requested and no reset, so that the cold part of the record is not
stored; the second without `info` and with every env truncated, so that the state goes out as the reset inside the step left it
(new target and episode in the cold part), while reward and info show the values before that reset.

Sizes: 32 800 = 1 025 tiles, the smallest batch on the row pass; 32 801: one env more, a ragged last tile of a single env.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _fresh(sizes, seed):
    from pioneer_amd import PioneerVectorEnv, EngineConfig
    envs, off = [], 0
    for m in sizes:
        envs.append(PioneerVectorEnv(m, device="cuda:0", seed=seed, env_id_offset=off,
                                     engine_config=EngineConfig(max_episode_steps=2, auto_reset=True)))
        off += m
    for e in envs:
        e.reset()
    return envs


def _step(envs, act, want_info):
    outs, off = [], 0
    for e in envs:
        m = e.num_envs
        outs.append([x.clone() for x in e.vector_step(act[off:off + m], want_info=want_info)])
        off += m
    return [torch.cat(parts) for parts in zip(*outs)]


@pytest.mark.parametrize("n", [32800, 32801])
def test_row_pass_form_equals_two_handles_without_the_row_pass_bit_for_bit(n):
    one = _fresh([n], seed=13)
    two = _fresh([n // 2, n - n // 2], seed=13)
    g = torch.Generator(device="cpu").manual_seed(n)
    amax = torch.from_numpy(one[0].a_max)
    names = ("obs", "reward", "done", "truncated", "info")
    for t, want_info in enumerate((True, False)):
        act = ((torch.rand(n, 6, generator=g) * 2 - 1) * amax).cuda()
        got, want = _step(one, act, want_info), _step(two, act, want_info)
        assert len(got) == (5 if want_info else 4)
        for name, a, b in zip(names, got, want):
            # bit for bit: the floats are compared as words, so a NaN or a signed zero cannot hide a difference
            a = a.view(torch.int32) if a.dtype == torch.float32 else a
            b = b.view(torch.int32) if b.dtype == torch.float32 else b
            assert torch.equal(a, b), f"{name} differs at step {t}"
        trunc = got[3].cpu().numpy()
        # (an env that came within done_distance in the first step starts over there and is not cut in the second)
        assert trunc.mean() > 0.99 if t == 1 else not trunc.any()
        assert torch.equal(one[0].get_state(), torch.cat([e.get_state() for e in two], dim=1)), f"state words differ at step {t}"
    w = one[0].get_state().cpu().numpy().view(np.uint32)
    assert np.all(w[23] >= 2), "every env was reset by the second step at the latest (episode 1 is the initial reset's)"
    for e in one + two:
        e.close()
