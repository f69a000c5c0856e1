"""tests/ppo_loss_ref.py — the float64 per-sample PPO loss the fused train-step kernel is held against (test_gpu_fused_loss.py)
— against float64 torch autograd of the torch formulation (PPOLearner.loss()'s arithmetic from the head rows on:
pioneer_amd.ppo.gaussian_logp / gaussian_kl / gaussian_entropy, torch.clamp / minimum / maximum), on the case table itself."""
import numpy as np
import pytest
import torch

import ppo_loss_ref as ref


def _autograd(head_p, head_v, rec, clip, vf_clip, vf_coeff, kl_c, ent_c):
    from pioneer_amd.ppo import gaussian_entropy, gaussian_kl, gaussian_logp
    t = lambda x: torch.from_numpy(np.asarray(x, np.float64))   # noqa: E731
    hp, hv = t(head_p).requires_grad_(True), t(head_v).requires_grad_(True)
    mb = {k: t(v) for k, v in rec.items()}
    mean, log_std, v = hp[:, :6], torch.clamp(hp[:, 6:12], -20.0, 2.0), hv[:, 0]
    logp = gaussian_logp(mb["actions"], mean, log_std)
    ratio = torch.exp(logp - mb["logp"])
    adv = mb["adv"]
    surr = torch.minimum(adv * ratio, adv * torch.clamp(ratio, 1 - clip, 1 + clip))
    kl = gaussian_kl(mb["mean"], mb["log_std"], mean, log_std)
    ent = gaussian_entropy(log_std)
    vf1 = (v - mb["vtarg"]) ** 2
    v_clipped = mb["values"] + torch.clamp(v - mb["values"], -vf_clip, vf_clip)
    vf = torch.maximum(vf1, (v_clipped - mb["vtarg"]) ** 2)
    total = (-surr + kl_c * kl + vf_coeff * vf - ent_c * ent).mean()
    total.backward()
    per_sample = {"neg_surr": -surr, "vf": vf, "kl": kl, "ent": ent}
    means = torch.stack([(-surr).mean(), vf.mean(), kl.mean(), ent.mean(), total])
    return ({k: x.detach().numpy() for k, x in per_sample.items()}, torch.stack([hp.grad, hv.grad]).numpy(), means.detach().numpy())


def _close(a, b, rtol=1e-12):
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all(np.abs(a - b) <= rtol * np.maximum(np.abs(b).max(), 1e-300)))


@pytest.mark.parametrize("row", ["moderate", "clamp"])
@pytest.mark.parametrize("B", [1, 65, 130])
def test_reference_equals_float64_autograd_on_the_case_table(row, B):
    tab = ref.make_table(row, B, seed=B)
    for kl_c, ent_c in ((ref.KL_COEFF, ref.ENT_COEFF), (0.0, 0.0)):
        r = ref.ppo_loss_ref(tab["head_p"], tab["head_v"], tab["rec"], kl_coeff=kl_c, ent_coeff=ent_c)
        per, g, means = _autograd(tab["head_p"], tab["head_v"], tab["rec"], ref.CLIP, ref.VF_CLIP, ref.VF_COEFF, kl_c, ent_c)
        for k in per:
            assert _close(r[k], per[k]), k
        assert r["g_head"].shape == (2, B, 16)
        for net in range(2):
            for s in range(B):                                 # sample by sample, relative to the sample's own largest entry
                assert _close(r["g_head"][net, s], g[net, s]), (net, s)
        assert np.allclose(r["means"], means, rtol=1e-12, atol=0.0)
        assert not r["g_head"][0, :, 12:].any() and not r["g_head"][1, :, 1:].any()         # the padding columns
    if row == "clamp":       # beyond the clamp: no gradient; on its bounds: the gradient passes
        r = ref.ppo_loss_ref(tab["head_p"], tab["head_v"], tab["rec"])
        assert not r["g_head"][0, :, 6:8].any() and bool(np.all(r["g_head"][0, :, 8:10] != 0.0))


def test_reference_follows_autograd_through_ties_and_clamp_bounds_of_random_records():
    """Away from the table: random heads and records with exact ties (ratio == 1, v == v_old, adv == 0) and raw log-stds on
    and beyond the clamp's bounds."""
    rng = np.random.RandomState(5)
    B = 97
    hp = np.zeros((B, 16)); hv = np.zeros((B, 16))
    hp[:, :6] = rng.randn(B, 6); hp[:, 6:12] = 0.7 * rng.randn(B, 6) - 0.5; hv[:, 0] = 3 * rng.randn(B)
    hp[0, 6:12] = [2.5, -21.0, 2.0, -20.0, 0.0, 1.0]
    ls = np.clip(hp[:, 6:12], -20, 2)
    rec = {"actions": hp[:, :6] + 1.5 * np.exp(ls) * rng.randn(B, 6), "mean": hp[:, :6] + 0.3 * np.exp(ls) * rng.randn(B, 6),
           "log_std": np.clip(ls + 0.2 * rng.randn(B, 6), -20, 2), "adv": rng.randn(B), "vtarg": 3 * rng.randn(B),
           "values": hv[:, 0] + 8 * rng.randn(B)}
    rec["actions"][0, :4] = hp[0, :4]; rec["mean"][0, :4] = hp[0, :4]; rec["log_std"][0, :4] = ls[0, :4]
    lp = ref._logp64(rec["actions"], hp[:, :6], ls)
    rec["logp"] = lp + 0.4 * rng.randn(B)
    rec["logp"][1] = lp[1]; rec["values"][2] = hv[2, 0]; rec["adv"][3] = 0.0
    r = ref.ppo_loss_ref(hp, hv, rec)
    assert r["ratio"][1] == 1.0 and r["dv"][2] == 0.0
    per, g, means = _autograd(hp, hv, rec, ref.CLIP, ref.VF_CLIP, ref.VF_COEFF, ref.KL_COEFF, ref.ENT_COEFF)
    for net in range(2):
        for s in range(B):
            assert _close(r["g_head"][net, s], g[net, s]), (net, s)
    assert np.allclose(r["means"], means, rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("row", ["moderate", "clamp"])
@pytest.mark.parametrize("B", [1, 63, 65, 130, 390])
def test_table_keeps_every_sample_off_the_boundaries(row, B):
    """The conditions that let the GPU tests compare EVERY sample (no allowance for samples near a clip boundary) hold for
    every row of every table those tests build (B = 390: the record a batch of 130 is gathered from)."""
    tab = ref.make_table(row, B, seed=B)
    r = ref.check_conditions(tab["head_p"], tab["head_v"], tab["rec"])
    # the ratio the table asked for is the ratio the reference sees (the old log-prob was rounded to float32)
    assert np.all(np.abs(r["ratio"] / tab["target"] - 1.0) < 1e-5)
    assert np.all(np.abs(r["dv"] - tab["dv_case"]) < 1e-5)
    if row == "clamp":
        rec = tab["rec"]
        assert np.array_equal(rec["actions"][:, :4], tab["head_p"][:, :4]) and np.array_equal(rec["mean"][:, :4], tab["head_p"][:, :4])
        assert np.array_equal(rec["log_std"][:, :4], np.clip(tab["head_p"][:, 6:10], -20, 2))


@pytest.mark.parametrize("row", ["moderate", "clamp"])
@pytest.mark.parametrize("B", [65, 130])
def test_table_populates_every_branch(row, B):
    tab = ref.make_table(row, B, seed=B)
    r = ref.ppo_loss_ref(tab["head_p"], tab["head_v"], tab["rec"])
    for name, mask in ref.branches(tab["rec"], r).items():
        assert int(mask.sum()) >= 1, name
    # every (ratio target, advantage sign) pair and every (value step, target offset) pair occurs
    sign = np.sign(tab["rec"]["adv"])
    assert len({(t, s) for t, s in zip(tab["target"], sign)}) == 14
    assert len({(a, b) for a, b in zip(tab["dv_case"], tab["vt_case"])}) == 28


def test_one_hot_batch_has_one_non_zero_row():
    tab = ref.make_table("clamp", 130, seed=130)
    srcs = ref.loud_rows(tab, 4)
    assert len(set(srcs)) == 4
    for k, src in zip((0, 63, 64, 129), srcs):
        rec = ref.one_hot(tab, k, src)
        r = ref.check_conditions(tab["head_p"], tab["head_v"], rec)
        r = ref.ppo_loss_ref(tab["head_p"], tab["head_v"], rec, kl_coeff=0.0, ent_coeff=0.0)
        others = np.arange(130) != k
        assert not r["g_head"][:, others].any()
        assert r["g_head"][0, k, :12].any() and r["g_head"][1, k, 0] != 0.0
        assert np.array_equal(r["g_head"].sum(1), r["g_head"][:, k])
