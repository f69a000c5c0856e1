"""The PPO loss inside the fused train-step kernel (mlp_tile_loss of csrc/pnr_mlp_forward.h: eight lanes per sample, the record
from global memory, from LDS or from registers) SAMPLE BY SAMPLE against the float64 reference of tests/ppo_loss_ref.py.

The model's last layers have W3 = 0, so every sample's head row is the bias b3 — known to the bit, asserted first — and the
reference needs no restatement of the nets.  The record comes from the reference's case table: every ratio target on both sides
of the surrogate's clip for both advantage signs, every value step on both sides of vf_clip, raw log-stds beyond and on the
clamp's bounds, and no sample near a boundary (tests/test_ppo_loss_ref_cpu.py), so every comparison below covers EVERY sample.

planes = 1 with HipMLP.w3_partials = False writes g_head [2][B][16] to the workspace: compared entry by entry (a).  For the other
modes g_head stays on the chip; its column sums are the last layer's bias gradients in the flat bucket (c), which a ONE-HOT batch
— one sample with a gradient, all others exactly zero — turns into that one sample's row: a mis-paired record or a dropped row at
a tile edge shows there for the register path (planes = 2) and the three-plane LDS path too.  The means are (b).

The measured err / bound ratios go to fused_loss_margins.json, next to the dynamics tests' margins (the _record_margin of
tests/test_gpu_dynamics.py; never part of a verdict)."""
import functools

import numpy as np
import pytest
import torch

import ppo_loss_ref as ref
from gpu_support import mlp_make as make, unpack_flat as _unpack_flat

pytestmark = pytest.mark.gpu
SENTINEL = -777.25


def _record_margin(case, figures):
    from test_gpu_dynamics import _record_margin as record
    record(case, None, None, file="fused_loss_margins.json", figures=figures)


def _setup(B, row, rows=None, planes=1):
    """make()'s model with W3 = 0 and b3 = the table's head row, packed; asserts the heads ARE b3, bit for bit."""
    from pioneer_amd.mlp import HipMLP
    model, mlp, obs, idx, _ = make(B, seed=B + 7 * planes, rows=rows)
    dev = obs.device
    with torch.no_grad():
        model.policy[4].weight.zero_(); model.value[4].weight.zero_()
        model.policy[4].bias.copy_(torch.tensor(ref.HEAD_ROWS[row], device=dev)); model.value[4].bias.fill_(ref.VALUE_B3)
    if planes != 1:
        mlp = HipMLP(model, B, dev, planes=planes)
    mlp.pack()
    hp, hv = ref.head_rows(row, B)
    heads = mlp.forward_nograd(obs, idx)
    assert torch.equal(heads[0].cpu(), torch.from_numpy(hp)) and torch.equal(heads[1].cpu(), torch.from_numpy(hv)), \
        f"planes {planes}: the heads of a W3 = 0 model are not its b3"
    return model, mlp, obs, idx


def _dev(rec, dev):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in rec.items()}


def _coeffs(dev, kl=ref.KL_COEFF, ent=ref.ENT_COEFF):
    return torch.tensor(kl, device=dev), torch.tensor(ent, device=dev)


def _step(mlp, obs, idx, rec, klc, entc, xs_in=None):
    dev = mlp.device
    means = torch.full((8,), float("nan"), device=dev)
    flat = torch.full((int(mlp.lib.pnr_mlp_grad_floats()),), float("nan"), device=dev)
    mlp.train_step(obs, idx, None, rec, klc, entc, ref.CLIP, ref.VF_CLIP, ref.VF_COEFF, means, 1e-3, flat_grad=flat, xs_in=xs_in)
    torch.cuda.synchronize()
    return means.double().cpu().numpy(), flat


# ---- (a) per sample: planes = 1, g_head in the workspace ---------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["idx", "rows", "xs_in"])
@pytest.mark.parametrize("B", [1, 63, 65, 130])          # one partial tile | a tile short by one | one over | two tiles plus two
@pytest.mark.parametrize("row", ["moderate", "clamp"])
def test_head_gradient_of_every_sample(row, B, path):
    """The three ways planes = 1 reaches the record: `idx` = global loads through the minibatch gather (R = 3 B record rows, a random
    subset in random order), `rows` = contiguous rows parked in LDS, `xs_in` = the same LDS path behind gather_epoch, on a
    minibatch that starts B rows into the gathered epoch (record slices that start on any float)."""
    R = B if path == "rows" else 3 * B
    model, mlp, obs, idx = _setup(B, row, rows=None if path == "rows" else R)
    dev = obs.device
    mlp.w3_partials = False                                # H2 and g_head leave the chip; layer 3's gradients come from the weight-gradient kernel
    tab = ref.make_table(row, R, seed=R)
    klc, entc = _coeffs(dev)
    ws = mlp._workspace()
    ws["g"] = torch.full((2 * B * 16 + 1024,), SENTINEL, device=dev)
    if path == "idx":
        rows = idx.cpu().numpy()
        means, flat = _step(mlp, obs, idx, _dev(tab["rec"], dev), klc, entc)
    elif path == "rows":
        rows = np.arange(B)
        means, flat = _step(mlp, obs, None, _dev(tab["rec"], dev), klc, entc)
    else:
        g = torch.Generator(device=dev).manual_seed(B)
        perm = torch.randperm(R, generator=g, device=dev)
        ga = mlp.gather_epoch(obs, perm, None, _dev(tab["rec"], dev))
        rows = perm[B:2 * B].cpu().numpy()
        means, flat = _step(mlp, None, None, {k: ga[k][B:2 * B] for k in mlp.REC_KEYS}, klc, entc, xs_in=ga["xs"][B:2 * B])
    want = ref.check_conditions(tab["head_p"][:B], tab["head_v"][:B], ref.take(tab["rec"], rows))
    got = ws["g"][:2 * B * 16].view(2, B, 16).double().cpu().numpy()
    assert bool((ws["g"][2 * B * 16:] == SENTINEL).all()), "written behind g_head [2][B][16]"
    assert np.all(np.isfinite(got))
    worst = 0.0
    for net in range(2):
        rowmax = np.abs(want["g_head"][net]).max(1, keepdims=True)
        err = np.abs(got[net] - want["g_head"][net])
        bound = 2e-4 * rowmax + 1e-9
        worst = max(worst, float((err / bound).max()))
    print(f"fused loss per sample [{row} B={B} {path}]: worst err / bound = {worst:.4f}")
    _record_margin(f"per_sample/{row}/B{B}/{path}", {"err_over_bound": worst, "bound": "2e-4 * row max + 1e-9"})
    for net in range(2):
        rowmax = np.abs(want["g_head"][net]).max(1, keepdims=True)
        bad = np.flatnonzero((np.abs(got[net] - want["g_head"][net]) > 2e-4 * rowmax + 1e-9).any(1))
        assert bad.size == 0, (net, bad[:8].tolist(), worst)              # EVERY sample: the table keeps them off the boundaries
    assert not got[0, :, 12:].any() and not got[1, :, 1:].any()           # padding columns exactly 0.0
    if row == "clamp":
        assert not got[0, :, 6:8].any()                                   # raw log-std beyond the clamp: no gradient, any sample
        assert bool(np.all(got[0, :, 8:10] != 0.0))                       # on a bound: it passes
    assert np.allclose(means[:5], want["means"], rtol=2e-5, atol=1e-5), (means[:5], want["means"])


# ---- (b), (c): the means and the last layer's bias gradient, every `planes`, in the trainer's default mode -----------------------
@functools.lru_cache(maxsize=None)
def _bucket_run(planes, row, B, hot):
    """One train_step on pre-gathered rows (xs_in; w3_partials on).  hot = None: the case table with the coefficients of (a);
    hot = k: the one-hot batch around sample k with kl_coeff = ent_coeff = 0.  Returns the loss means, the twelve gradients of
    the flat bucket and the reference."""
    model, mlp, obs, _ = _setup(B, row, planes=planes)
    dev = obs.device
    tab = ref.make_table(row, B, seed=B)
    if hot is None:
        rec, kl, ent = tab["rec"], ref.KL_COEFF, ref.ENT_COEFF
    else:
        src = ref.loud_rows(tab, 4)[(0, 63, 64, 129).index(hot)]
        rec, kl, ent = ref.one_hot(tab, hot, src), 0.0, 0.0
    klc, entc = _coeffs(dev, kl, ent)
    ga = mlp.gather_epoch(obs, torch.arange(B, device=dev), None, _dev(rec, dev))
    means, flat = _step(mlp, None, None, {k: ga[k] for k in mlp.REC_KEYS}, klc, entc, xs_in=ga["xs"])
    want = ref.check_conditions(tab["head_p"], tab["head_v"], rec)
    want = ref.ppo_loss_ref(tab["head_p"], tab["head_v"], rec, kl_coeff=kl, ent_coeff=ent)
    return means, [g.double().cpu().numpy() for g in _unpack_flat(flat)], want


@pytest.mark.parametrize("planes", [1, 2, 3])
@pytest.mark.parametrize("B", [63, 130])
@pytest.mark.parametrize("row", ["moderate", "clamp"])
def test_loss_means(planes, row, B):
    means, _, want = _bucket_run(planes, row, B, None)
    tol = 1e-5 + 2e-5 * np.abs(want["means"])
    worst = float((np.abs(means[:5] - want["means"]) / tol).max())
    print(f"fused loss means [planes={planes} {row} B={B}]: worst err / (atol + rtol |ref|) = {worst:.4f}")
    _record_margin(f"means/planes{planes}/{row}/B{B}", {"err_over_bound": worst, "bound": "1e-5 + 2e-5 |ref|"})
    assert np.allclose(means[:5], want["means"], rtol=2e-5, atol=1e-5), (means[:5], want["means"])
    total = means[0] + ref.KL_COEFF * means[2] + ref.VF_COEFF * means[1] - ref.ENT_COEFF * means[3]
    assert np.isclose(means[4], total, rtol=2e-5, atol=1e-5), (means[4], total)


# relative to the largest entry of the row: 2^-8 for planes = 1 (the tile rounds its head gradients to bf16 before layer 3's
# products), SPLIT_TOL's gradient bound for the split operands
B3_BOUND = {1: 2.0 ** -8, 2: 1e-4, 3: 1e-4}


@pytest.mark.parametrize("planes", [1, 2, 3])
@pytest.mark.parametrize("hot", [None, 0, 63, 64, 129])
@pytest.mark.parametrize("row", ["moderate", "clamp"])
def test_last_layer_bias_gradient(planes, row, hot):
    """The b3 entries of both nets in the flat bucket = the column sums of g_head; on a one-hot batch = the one sample's row."""
    B = 130
    _, grads, want = _bucket_run(planes, row, B, hot)
    col = want["g_head"].sum(1)                                          # [2][16]
    if hot is not None:
        assert np.array_equal(col, want["g_head"][:, hot]) and col[0, :12].any() and col[1, 0] != 0.0
    fig = {}
    for net, (got, ref_row) in enumerate(((grads[5], col[0, :12]), (grads[11], col[1, :1]))):
        err = np.abs(got - ref_row)
        fig["policy" if net == 0 else "value"] = float(err.max() / (B3_BOUND[planes] * np.abs(ref_row).max()))
    print(f"fused loss b3 gradient [planes={planes} {row} hot={hot}]: err / bound = {fig}")
    _record_margin(f"b3/planes{planes}/{row}/{'table' if hot is None else 'hot%d' % hot}", dict(fig, bound=f"{B3_BOUND[planes]:.3e} * row max"))
    for net, (got, ref_row) in enumerate(((grads[5], col[0, :12]), (grads[11], col[1, :1]))):
        assert np.all(np.abs(got - ref_row) <= B3_BOUND[planes] * np.abs(ref_row).max()), (net, got, ref_row)
    if row == "clamp":
        assert not grads[5][6:8].any()                                   # beyond the clamp
    # W3 = 0: nothing reaches the layers below
    for i in (0, 1, 2, 3, 6, 7, 8, 9):
        assert not grads[i].any(), i
    assert grads[4].any() and grads[10].any()                            # layer 3's own weights do get a gradient
