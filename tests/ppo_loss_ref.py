"""A float64 restatement of the PPO loss per sample, and the case table the fused train-step kernel is tested on.

`ppo_loss_ref` takes the two nets' head rows and a rollout record and returns, per sample, -surrogate, the value loss, KL and
entropy, the gradient of the batch-mean total loss with respect to the heads ([2][B][16], padding columns zero) and the five
means.  The derivatives are written out by hand with the semantics of PPOLearner.loss() under torch autograd: clamp passes the
gradient on the closed interval, minimum / maximum split a tie, the clipped branch is constant outside its range
(tests/test_ppo_loss_ref_cpu.py holds it against float64 autograd to 1e-12).

`make_table` builds records that put every sample on a chosen side of every branch, and far enough from each boundary that a
float32 kernel and this reference cannot disagree about the side (`check_conditions`), so that NO sample has to be exempted
from a per-sample comparison.  The heads are the same row for every sample — a net whose last layer has W3 = 0 emits its bias
b3 whatever the input — which makes them known to the bit."""
import math

import numpy as np

CLIP, VF_CLIP, VF_COEFF = 0.3, 10.0, 1.0
KL_COEFF, ENT_COEFF = 0.37, 0.013                     # the stand-alone loss kernel's test uses the same two
RATIO_TARGETS = (0.4, 0.65, 0.75, 1.0, 1.25, 1.35, 2.0)   # both sides of 1 -+ clip, near and far, and the middle
DV_CASES = (-15.0, -10.5, -9.5, 0.0, 9.5, 10.5, 15.0)     # v - v_old against vf_clip = 10
VT_CASES = (-20.0, -3.0, 3.0, 20.0)                        # vtarg - v
_MEANS = (0.5, -0.4, 0.6, -0.55, 0.45, -0.5)
HEAD_ROWS = {
    "moderate": _MEANS + (-1.0, -0.5, 0.0, 0.3, 0.7, 1.0),
    "clamp": _MEANS + (2.5, -21.0, 2.0, -20.0, 0.0, 1.0),  # raw log-stds beyond and ON the clamp's bounds (dimensions 0..3)
}
VALUE_B3 = 0.71
LOG_2PI = math.log(2.0 * math.pi)
REC_KEYS = ("actions", "logp", "mean", "log_std", "adv", "vtarg", "values")


def head_rows(row, n):
    """The heads of n samples of a W3 = 0 model: policy rows = b3 (12 entries, 4 zero padding columns), value rows = (v, 0 ..)."""
    hp = np.zeros((n, 16), np.float32)
    hv = np.zeros((n, 16), np.float32)
    hp[:, :12] = np.asarray(HEAD_ROWS[row], np.float32)
    hv[:, 0] = np.float32(VALUE_B3)
    return hp, hv


def _logp64(actions, mean, ls):
    z = (actions - mean) * np.exp(-ls)
    return (-0.5 * z * z - ls - 0.5 * LOG_2PI).sum(-1)


def ppo_loss_ref(head_p, head_v, rec, clip=CLIP, vf_clip=VF_CLIP, vf_coeff=VF_COEFF, kl_coeff=KL_COEFF, ent_coeff=ENT_COEFF):
    f8 = lambda x: np.asarray(x, np.float64)   # noqa: E731
    hp, hv = f8(head_p), f8(head_v)
    B = hp.shape[0]
    a, m0, l0 = f8(rec["actions"]), f8(rec["mean"]), f8(rec["log_std"])
    adv, lp0, vt, v0 = f8(rec["adv"]), f8(rec["logp"]), f8(rec["vtarg"]), f8(rec["values"])
    m, raw, v = hp[:, :6], hp[:, 6:12], hv[:, 0]
    # ---- policy
    passes = (raw >= -20.0) & (raw <= 2.0)                # clamp: gradient on the closed interval
    ls = np.clip(raw, -20.0, 2.0)
    si = np.exp(-ls)
    z = (a - m) * si
    logp = (-0.5 * z * z - ls - 0.5 * LOG_2PI).sum(-1)
    ratio = np.exp(logp - lp0)
    inrange = (ratio >= 1.0 - clip) & (ratio <= 1.0 + clip)
    s1, s2 = adv * ratio, adv * np.clip(ratio, 1.0 - clip, 1.0 + clip)
    surr = np.minimum(s1, s2)
    w1 = np.where(s1 < s2, 1.0, np.where(s1 == s2, 0.5, 0.0))     # minimum: the smaller argument takes the gradient, a tie splits it
    dsurr = w1 * s1 + (1.0 - w1) * np.where(inrange, s1, 0.0)      # d surr / d logp  (d s1 / d logp = s1, d s2 / d logp = s1 inside the range)
    ivar = si * si
    dm = m0 - m
    q = (np.exp(2.0 * l0) + dm * dm) * ivar
    kl = (ls - l0 + 0.5 * q - 0.5).sum(-1)
    ent = (ls + 0.5 * (LOG_2PI + 1.0)).sum(-1)
    g = np.zeros((2, B, 16))
    g[0, :, :6] = (-dsurr[:, None] * z * si + kl_coeff * (-dm * ivar)) / B
    g[0, :, 6:12] = np.where(passes, -dsurr[:, None] * (z * z - 1.0) + kl_coeff * (1.0 - q) - ent_coeff, 0.0) / B
    # ---- value
    e1 = v - vt
    dv = v - v0
    vin = (dv >= -vf_clip) & (dv <= vf_clip)
    e2 = v0 + np.clip(dv, -vf_clip, vf_clip) - vt
    f1, f2 = e1 * e1, e2 * e2
    vf = np.maximum(f1, f2)
    g1, g2 = 2.0 * e1, np.where(vin, 2.0 * e2, 0.0)
    dvf = np.where(f1 > f2, g1, np.where(f1 < f2, g2, 0.5 * (g1 + g2)))
    g[1, :, 0] = vf_coeff * dvf / B
    total = -surr + kl_coeff * kl + vf_coeff * vf - ent_coeff * ent
    means = np.array([(-surr).mean(), vf.mean(), kl.mean(), ent.mean(), total.mean()])
    return {"neg_surr": -surr, "vf": vf, "kl": kl, "ent": ent, "g_head": g, "means": means,
            "ratio": ratio, "inrange": inrange, "dsurr": dsurr, "dv": dv, "f1": f1, "f2": f2}


def make_table(row, n, seed=0):
    """n record rows for the head row `row` ("moderate" / "clamp").  Sample i takes ratio target i % 7 with advantage sign
    (i // 7) % 2 and value case (v - v_old = DV_CASES[i % 7], vtarg - v = VT_CASES[(i // 7) % 4]): periods 14 and 28, neither a
    divisor of the 64-sample tile, so a tile's slots see the cases in shifting order; the magnitudes (actions, old means and
    log-stds, |adv|) are random, so no two samples carry the same policy record.  The ratio is set through the old log-prob:
    logp_old = float32(logp64 - ln(target)) with logp64 this reference's log-prob of the float32 inputs."""
    rng = np.random.RandomState(1000 + seed)
    hp, hv = head_rows(row, n)
    mean, raw = hp[:, :6].astype(np.float64), hp[:, 6:12].astype(np.float64)
    ls = np.clip(raw, -20.0, 2.0)
    u = lambda: rng.uniform(-1.0, 1.0, (n, 6))   # noqa: E731
    actions = (mean + 1.5 * np.exp(ls) * u()).astype(np.float32)
    mean_old = (mean + 0.3 * np.exp(ls) * u()).astype(np.float32)
    ls_old = np.clip(ls + 0.2 * u(), -20.0, 2.0).astype(np.float32)
    if row == "clamp":
        # the four extreme dimensions: action == old mean == mean and old log-std == clamp(raw), so z = 0, m0 - m = 0, q = 1 and
        # nothing overflows (exp(20) scales every deviation there)
        actions[:, :4] = hp[:, :4]; mean_old[:, :4] = hp[:, :4]; ls_old[:, :4] = ls[:, :4].astype(np.float32)
    i = np.arange(n)
    target = np.asarray(RATIO_TARGETS)[i % 7]
    sign = np.where((i // 7) % 2 == 0, 1.0, -1.0)
    adv = (sign * rng.uniform(0.5, 2.0, n)).astype(np.float32)
    logp = (_logp64(actions.astype(np.float64), mean, ls) - np.log(target)).astype(np.float32)
    dv = np.asarray(DV_CASES)[i % 7]
    dvt = np.asarray(VT_CASES)[(i // 7) % 4]
    v = np.float32(VALUE_B3)
    values = (np.float64(v) - dv).astype(np.float32)
    values[dv == 0.0] = v                                    # v == v_old exactly: the maximum's tie
    vtarg = (np.float64(v) + dvt).astype(np.float32)
    rec = {"actions": actions, "logp": logp, "mean": mean_old, "log_std": ls_old, "adv": adv, "vtarg": vtarg, "values": values}
    return {"row": row, "head_p": hp, "head_v": hv, "rec": rec, "target": target, "dv_case": dv, "vt_case": dvt}


def take(rec, rows):
    return {k: np.ascontiguousarray(rec[k][rows]) for k in REC_KEYS}


def check_conditions(head_p, head_v, rec, clip=CLIP, vf_clip=VF_CLIP):
    """The conditions under which no sample needs an allowance, asserted on the reference itself for EVERY sample: the float64
    ratio of the float32-rounded inputs is at least 1e-3 away from 1 -+ clip, the value step is not within 1e-3 of +-vf_clip,
    and a sample whose value step is clipped has |f1 - f2| >= 1e-3 max(f1, f2) (the maximum's choice is not a near-tie)."""
    r = ppo_loss_ref(head_p, head_v, rec, clip, vf_clip)
    assert np.all(np.isfinite(r["g_head"])) and np.all(np.isfinite(r["means"]))
    assert np.all(np.abs(r["ratio"] - (1.0 - clip)) >= 1e-3) and np.all(np.abs(r["ratio"] - (1.0 + clip)) >= 1e-3)
    assert np.all(np.abs(np.abs(r["dv"]) - vf_clip) >= 1e-3)
    clipped = np.abs(r["dv"]) > vf_clip
    assert np.all(np.abs(r["f1"] - r["f2"])[clipped] >= 1e-3 * np.maximum(r["f1"], r["f2"])[clipped])
    return r


def branches(rec, r):
    """Which samples sit in which branch of the loss (boolean masks over the samples)."""
    adv = np.asarray(rec["adv"], np.float64)
    clipped_v = np.abs(r["dv"]) > VF_CLIP
    return {
        "surrogate clipped, adv > 0": (r["dsurr"] == 0.0) & (adv > 0) & ~r["inrange"],
        "surrogate clipped, adv < 0": (r["dsurr"] == 0.0) & (adv < 0) & ~r["inrange"],
        "unclipped below the range": (r["dsurr"] != 0.0) & (r["ratio"] < 1.0 - CLIP),
        "unclipped above the range": (r["dsurr"] != 0.0) & (r["ratio"] > 1.0 + CLIP),
        "inside the range": r["inrange"],
        "value clipped and chosen": clipped_v & (r["f2"] > r["f1"]),
        "value clipped and not chosen": clipped_v & (r["f1"] > r["f2"]),
        "value unclipped": ~clipped_v & (r["dv"] != 0.0),
        "v == v_old": r["dv"] == 0.0,
    }


def one_hot(table, k, src):
    """The table's batch with every sample silenced — adv = 0 and vtarg = v = v_old, so with kl_coeff = ent_coeff = 0 its head
    gradient is exactly zero — except sample k, which carries record row `src` of the table."""
    rec = {key: val.copy() for key, val in table["rec"].items()}
    keep = {key: val[src].copy() for key, val in rec.items()}
    rec["adv"][:] = 0.0
    rec["vtarg"][:] = np.float32(VALUE_B3); rec["values"][:] = np.float32(VALUE_B3)
    for key in REC_KEYS:
        rec[key][k] = keep[key]
    return rec


def loud_rows(table, count):
    """`count` different record rows of the table whose policy AND value gradients are non-zero (an unclipped surrogate, a value
    branch that passes the gradient): what a one-hot batch is made of."""
    r = ppo_loss_ref(table["head_p"], table["head_v"], table["rec"], kl_coeff=0.0, ent_coeff=0.0)
    ok = np.flatnonzero((r["dsurr"] != 0.0) & (r["g_head"][1, :, 0] != 0.0))
    assert ok.size >= count
    return [int(j) for j in ok[np.linspace(0, ok.size - 1, count).astype(int)]]
