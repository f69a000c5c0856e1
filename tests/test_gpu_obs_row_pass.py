"""step_kernel's row-ordered obs path (obs_tile_rows_out, pnr_device.h): linear entries first, then the sin / cos of the tile's
32 x 24 arguments in row order, each 1-KiB chunk of the tile stored as soon as its rows are complete.

What the path must keep, whatever lane evaluates an argument and whenever its chunk leaves: every sin / cos column of a returned
row is, bit for bit, the engine's own function of that row's argument column (pnr_diag_sincos runs sincos_bounded / sincos_any
on the same device), nothing is written past the batch's n * 137 floats, and an obs pointer that is not 16-byte aligned gets the
same rows.  pnr_step / pnr_rollout are called through ctypes on raw device pointers, as bench.py calls them.

pnr_step takes the row pass where a launch has more than one wave per SIMD (step_row_pass, pnr_api.hip: 32 768 < n <= 65 536) and
obs_tile_out below; pnr_rollout always takes obs_tile_out.  SIZES are on the obs_tile_out side of that rule, ROW_SIZES on the row
pass's side with the same last tiles; both sides must hold the same properties.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

OBS = 137
SPARE_ROWS = 64
SENTINEL = 0x7FC5A5A5          # a NaN payload no kernel arithmetic produces
STEPS = 3
# (argument columns, bounded): cos goes to columns + 6, sin to columns + 12
TRIG = [(0, 1), (54, 1), (72, 1), (90, 1), (108, 0)]
SIZES = [1, 23, 31, 33, 129, 2055]   # one pair; a tile that ends inside a chunk; ragged tiles; a second workgroup; many workgroups
ROW_BASE = 32768                      # 1 024 full tiles = one wave per SIMD: the row pass runs above it
ROW_SIZES = [ROW_BASE + k for k in (1, 23, 31, 33)]     # the last tile: one pair; ends inside a chunk; one env short; a tile and a pair


def _vp(t, byte_offset=0):
    return C.c_void_p(t.data_ptr() + byte_offset)


def _actions(n, a_max):
    """[STEPS, n, 6], finite: 0, +-a_max, the two sides of sincos_any's threshold, far beyond it and in-range values, laid out so
    that neighbouring joints and envs (the lanes of one wave in the row pass) take different branches."""
    e = np.arange(n)[None, :, None]
    j = np.arange(6)[None, None, :]
    t = np.arange(STEPS)[:, None, None]
    pick = (5 * e + 3 * j + t) % 9
    rnd = np.random.default_rng(4).uniform(-1.0, 1.0, (STEPS, n, 6)).astype(np.float32) * a_max
    am = np.broadcast_to(a_max, (STEPS, n, 6))
    table = [np.zeros_like(rnd), am, -am, np.full_like(rnd, 131072.0), np.full_like(rnd, 131073.0), np.full_like(rnd, 1.0e6),
             np.full_like(rnd, -131073.0), rnd, 0.5 * rnd]
    return np.choose(pick, table).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _run(n, rollout, offset_floats=0):
    """STEPS steps (max_episode_steps = 2: step 2 truncates and auto-resets) into obs buffers with one float in front of the obs
    pointer's 16-byte slot and SPARE_ROWS rows behind the batch, all pre-filled with SENTINEL.  Returns the raw buffers as uint32
    [STEPS or 1][4 + rows * 137], the truncated flags, which envs were re-drawn (done or truncated) and the actions."""
    from pioneer_amd import PioneerVectorEnv, EngineConfig, _lib
    env = PioneerVectorEnv(n, device="cuda:0", seed=21, engine_config=EngineConfig(auto_reset=True, max_episode_steps=2))
    env.reset()
    act = torch.from_numpy(_actions(n, env.a_max)).cuda()
    T = STEPS if rollout else 1
    rows = T * n + SPARE_ROWS
    bufs = [torch.full((4 + rows * OBS,), SENTINEL, dtype=torch.int32, device="cuda:0") for _ in range(STEPS // T)]
    rew = torch.empty((STEPS, n), dtype=torch.float32, device="cuda:0")
    done = torch.empty((STEPS, n), dtype=torch.uint8, device="cuda:0")
    trunc = torch.empty((STEPS, n), dtype=torch.uint8, device="cuda:0")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    first = 4 * (4 + offset_floats)            # bytes: the obs pointer is the buffer's float 4 (16-byte aligned) + offset_floats
    for k, b in enumerate(bufs):
        if rollout:
            rc = env.lib.pnr_rollout(env._h, T, _vp(act), _vp(b, first), _vp(rew), _vp(done), _vp(trunc), st)
        else:
            rc = env.lib.pnr_step(env._h, _vp(act[k]), _vp(b, first), _vp(rew[k]), _vp(done[k]), _vp(trunc[k]), None, st)
        _lib.check(rc, env._h)
    torch.cuda.synchronize()
    raw = [b.cpu().numpy().view(np.uint32) for b in bufs]
    out = (raw, trunc.cpu().numpy(), (done | trunc).cpu().numpy() != 0, act.cpu().numpy())
    env.close()
    return out


def _steps(raw, n, offset_floats=0):
    """the STEPS returned batches [n, 137] (uint32 views) out of the raw buffers"""
    lo = 4 + offset_floats
    if len(raw) == 1:
        return [raw[0][lo + t * n * OBS: lo + (t + 1) * n * OBS].reshape(n, OBS) for t in range(STEPS)]
    return [b[lo: lo + n * OBS].reshape(n, OBS) for b in raw]


def _sincos(x_bits, bounded):
    from pioneer_amd import _lib
    lib = _lib.load_library()
    x = torch.from_numpy(np.ascontiguousarray(x_bits).view(np.float32)).cuda()
    s = torch.empty_like(x); c = torch.empty_like(x)
    _lib.check(lib.pnr_diag_sincos(_vp(x), _vp(s), _vp(c), x.numel(), int(bounded), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return s.cpu().numpy().view(np.uint32), c.cpu().numpy().view(np.uint32)


def _check_rows(obs_bits, what):
    """every trig column of every row = the engine's function of the row's own argument column, bit for bit"""
    assert not (obs_bits == SENTINEL).any(), f"{what}: an entry of the batch was not written"
    for col, bounded in TRIG:
        arg = obs_bits[:, col:col + 6]
        s, c = _sincos(arg.reshape(-1), bounded)
        assert np.array_equal(obs_bits[:, col + 6:col + 12].reshape(-1), c), f"{what}: cos of columns {col}:{col + 6}"
        assert np.array_equal(obs_bits[:, col + 12:col + 18].reshape(-1), s), f"{what}: sin of columns {col}:{col + 6}"


def _check_actions_shown(steps, redrawn, act, what):
    """the `a` columns hold the action just given (an env re-drawn at this step shows 0): ties the rows to the inputs, so the ocml
    branch of sincos_any was really taken by some arguments and not by their neighbours"""
    for t, o in enumerate(steps):
        keep = ~redrawn[t]
        assert np.array_equal(o[:, 108:114].view(np.float32)[keep], act[t][keep]), f"{what}: action columns at step {t}"
    shown = np.abs(np.concatenate([o[:, 108:114].view(np.float32).reshape(-1) for o in steps]))
    if shown.size >= 24:
        assert (shown > 131072.0).any() and (shown <= 131072.0).any()


@pytest.mark.parametrize("rollout", [False, True], ids=["step", "rollout"])
@pytest.mark.parametrize("n", SIZES + ROW_SIZES)
def test_trig_columns_are_the_engines_function_of_the_rows_own_arguments(n, rollout):
    raw, trunc, redrawn, act = _run(n, rollout)
    steps = _steps(raw, n)
    assert trunc[1].any() and not trunc[0].any()       # the truncation and the auto-reset fall inside the run
    for t, o in enumerate(steps):
        _check_rows(o, f"n={n} step {t}")
    _check_actions_shown(steps, redrawn, act, f"n={n}")


@pytest.mark.parametrize("n", [33, 1, ROW_BASE + 33, ROW_BASE + 1])
def test_nothing_is_written_beyond_the_batch(n):
    raw = _run(n, False)[0]
    for t, b in enumerate(raw):
        assert (b[:4] == SENTINEL).all(), f"step {t}: written in front of the obs pointer"
        assert (b[4 + n * OBS:] == SENTINEL).all(), f"step {t}: written at or beyond n * 137"
    raw = _run(n, True)[0]
    assert (raw[0][:4] == SENTINEL).all() and (raw[0][4 + STEPS * n * OBS:] == SENTINEL).all()


@pytest.mark.parametrize("n", [33, ROW_BASE + 33])
def test_unaligned_obs_pointer_gets_the_same_rows(n):
    raw, _, redrawn, act = _run(n, False, 1)
    steps = _steps(raw, n, 1)
    for t, (b, o) in enumerate(zip(raw, steps)):
        assert (b[:5] == SENTINEL).all(), f"step {t}: the float in front of the obs pointer was written"
        assert (b[5 + n * OBS:] == SENTINEL).all(), f"step {t}: written at or beyond n * 137"
        _check_rows(o, f"unaligned, step {t}")
    _check_actions_shown(steps, redrawn, act, "unaligned")
    # same seed, same actions: the aligned run's rows
    for o, ref in zip(steps, _steps(_run(n, False)[0], n)):
        assert np.array_equal(o, ref)
