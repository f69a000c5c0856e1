"""A float64 restatement of the learner's two MLPs — forward, backward-data and the six weight gradients per net — and what the
element-by-element tests of the weight-gradient kernels are made of (tests/test_gpu_mlp_wgrad.py; this module is held against
float64 torch autograd by tests/test_mlp_grad_ref_cpu.py).

`backward_ref` is the chain; with rounding="bf16" it rounds exactly where the bf16 kernels do (weights, inputs, stored
activations, the head gradients and the propagated gradients) and is what tests/test_gpu_mlp.py calls `emulate`.  `gemm_ref` is
one weight-gradient product with its sum of absolute terms, the unit every dense bound is stated in.  `planes_to_f64` reads a
stored 16-bit operand buffer as the number it stands for (include/pioneer_amd.h, pnr_mlp_pack).  `make_table_general`,
`silence`, `loud` and `one_hot_general` are tests/ppo_loss_ref.py's case table and one-hot batch for a model whose heads differ
from sample to sample.  `mlp_slicing` restates how a batch is cut into the weight-gradient kernel's slices."""
import numpy as np
import torch

import ppo_loss_ref as lref

IN, IN_PAD, HID, HEAD = 137, 144, 256, 16
WG_CHUNK, MAX_SLICES = 64, 32
# the power-of-two scales of the fp16 planes (planes = 2): activations, net inputs, weights (Fmt<2>::kSW); gradients: grad_scale(B)
SCALE_ACT, SCALE_INPUT, SCALE_WEIGHT = 2.0 ** 8, 2.0 ** 4, 2.0 ** 8


def bf(x):
    """rounded to bf16, as float64"""
    return x.to(torch.bfloat16).double()


def mlp_slicing(B):
    """(slices, rows per slice) of a batch of B samples: at most one slice per 64-sample chunk, at most 32 slices, whole chunks"""
    want = max(1, min((B + WG_CHUNK - 1) // WG_CHUNK, MAX_SLICES))
    rows = (B + want - 1) // want
    rows = (rows + WG_CHUNK - 1) // WG_CHUNK * WG_CHUNK
    return (B + rows - 1) // rows, rows


def grad_scale(B):
    """what the gradient planes of planes = 2 are stored multiplied by: 4 * 2^ceil(log2 B)"""
    g, n = 4.0, 1
    while n < B:
        g, n = g * 2.0, n * 2
    return g


def linears(net):
    """(W1, b1, W2, b2, W3, b3) of one net, detached"""
    return [t.detach() for l in net if isinstance(l, torch.nn.Linear) for t in (l.weight, l.bias)]


def backward_ref(model, x, g_head, rounding):
    """Per net a dict of float64 tensors: x [B, 137], h1, h2 [B, 256], head [B, 16] (padding columns zero) and — when g_head
    [2, B, 16] is given — g [B, 16] (the head gradient as the products see it, padding columns zero), dz2, dz1 [B, 256], grads
    (dW1 [256, 137], db1, dW2, db2, dW3 [n3, 256], db3) and abs: the sum of the absolute terms behind every entry of h1, h2
    (pre-activation, bias included), dz2 and dz1 (sum |g| |w| (1 + h^2): the product times the tanh derivative 1 - h^2, every term of
    the expanded expression taken absolute).
    rounding = "bf16": rounded where the bf16 kernels round; None: plain float64."""
    assert rounding in ("bf16", None)
    r = bf if rounding == "bf16" else (lambda t: t.double())
    xb = r(x)
    out = []
    for n, net in enumerate((model.policy, model.value)):
        W1, b1, W2, b2, W3, b3 = linears(net)
        n3 = W3.shape[0]
        W1r, W2r, W3r = r(W1), r(W2), r(W3)
        h1 = r(torch.tanh(xb @ W1r.t() + b1.double()))
        h2 = r(torch.tanh(h1 @ W2r.t() + b2.double()))
        head = torch.zeros(x.shape[0], HEAD, dtype=torch.float64, device=x.device)
        head[:, :n3] = h2 @ W3r.t() + b3.double()
        res = {"x": xb, "h1": h1, "h2": h2, "head": head,
               "abs": {"h1": xb.abs() @ W1r.abs().t() + b1.double().abs(), "h2": h1.abs() @ W2r.abs().t() + b2.double().abs()}}
        if g_head is not None:
            gb = r(g_head[n])[:, :n3]
            dz2 = r((gb @ W3r) * (1 - h2 * h2))
            dz1 = r((dz2 @ W2r) * (1 - h1 * h1))
            g = torch.zeros_like(head)
            g[:, :n3] = gb
            res.update(g=g, dz2=dz2, dz1=dz1, grads=[dz1.t() @ xb, dz1.sum(0), dz2.t() @ h1, dz2.sum(0), gb.t() @ h2, gb.sum(0)])
            res["abs"].update(dz2=(gb.abs() @ W3r.abs()) * (1 + h2 * h2), dz1=(dz2.abs() @ W2r.abs()) * (1 + h1 * h1))
        out.append(res)
    return out


def emulate(model, x, g_head):
    """float64 restatement with the kernels' bf16 rounding points.  Returns heads [2][B][16] and 12 gradients."""
    nets = backward_ref(model, x, g_head, "bf16")
    return torch.stack([n["head"] for n in nets]), [g for n in nets for g in n["grads"]]


def gemm_ref(a, b):
    """(a^T b, |a|^T |b|) in float64: a weight-gradient product over the samples (rows) and its sum of absolute terms"""
    a, b = a.double(), b.double()
    return a.t() @ b, a.abs().t() @ b.abs()


def planes_to_f64(buf, planes, kind, B):
    """The float64 value a stored 16-bit operand buffer [planes, ...] (bf16 element type) stands for: planes = 1 the bf16 value,
    3 the sum of the three bf16 planes, 2 the sum of the two fp16 planes over the tensor's power-of-two scale — kind "act"
    (2^8), "input" (2^4), "weight" (2^8) or "grad" (grad_scale(B))."""
    assert buf.dtype == torch.bfloat16 and buf.shape[0] == planes and planes in (1, 2, 3)
    if planes != 2:
        return buf.double().sum(0)                     # (a sum of at most three bf16 numbers is exact in float64)
    scale = {"act": SCALE_ACT, "input": SCALE_INPUT, "weight": SCALE_WEIGHT, "grad": grad_scale(B)}[kind]
    return buf.view(torch.float16).double().sum(0) / scale


def split_planes(v, planes, kind, B):
    """The CPU statement of the kernels' split of float32 values into [planes, ...] 16-bit planes (bf16 element type)."""
    v = v.float()
    if planes == 2:
        scale = {"act": SCALE_ACT, "input": SCALE_INPUT, "weight": SCALE_WEIGHT, "grad": grad_scale(B)}[kind]
        s = torch.clamp(v * scale, -65504.0, 65504.0)
        p0 = s.to(torch.float16)
        p1 = (s - p0.float()).to(torch.float16)
        return torch.stack([p0, p1]).view(torch.bfloat16)
    out, rest = [], v.clone()
    for _ in range(planes):
        p = rest.to(torch.bfloat16)
        out.append(p)
        rest = rest - p.float()
    return torch.stack(out)


# ---- the PPO record of a model whose heads differ per sample -------------------------------------------------------------------------
LOUD_DV, LOUD_VT = 3.0, 3.0          # the hot sample's value step v - v_old (inside vf_clip) and vtarg - v
SILENT_DV, SILENT_VT = 15.0, 20.0    # a silent sample's: the branch "value clipped and chosen", whose gradient is exactly zero


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, np.float64).astype(np.float32))


def make_table_general(head_p, head_v, seed=0):
    """ppo_loss_ref.make_table for per-sample heads [B, 16] (float64): sample i takes ratio target i % 7 with advantage sign
    (i // 7) % 2 and the value case (DV_CASES[i % 7], VT_CASES[(i // 7) % 4]) around ITS OWN heads; random magnitudes."""
    hp, hv = np.asarray(head_p, np.float64), np.asarray(head_v, np.float64)
    n = hp.shape[0]
    rng = np.random.RandomState(2000 + seed)
    mean, ls = hp[:, :6], np.clip(hp[:, 6:12], -20.0, 2.0)
    u = lambda: rng.uniform(-1.0, 1.0, (n, 6))   # noqa: E731
    actions = _f32(mean + 1.5 * np.exp(ls) * u())
    mean_old = _f32(mean + 0.3 * np.exp(ls) * u())
    ls_old = _f32(np.clip(ls + 0.2 * u(), -20.0, 2.0))
    i = np.arange(n)
    target = np.asarray(lref.RATIO_TARGETS)[i % 7]
    sign = np.where((i // 7) % 2 == 0, 1.0, -1.0)
    adv = _f32(sign * rng.uniform(0.5, 2.0, n))
    logp = _f32(lref._logp64(actions.astype(np.float64), mean, ls) - np.log(target))
    dv = np.asarray(lref.DV_CASES)[i % 7]
    dvt = np.asarray(lref.VT_CASES)[(i // 7) % 4]
    rec = {"actions": actions, "logp": logp, "mean": mean_old, "log_std": ls_old, "adv": adv,
           "vtarg": _f32(hv[:, 0] + dvt), "values": _f32(hv[:, 0] - dv)}
    return {"head_p": hp, "head_v": hv, "rec": rec, "target": target, "dv_case": dv, "vt_case": dvt}


def silence(rec, heads_v):
    """A copy of the record in which EVERY sample is silent: adv = 0 (the surrogate and its gradient vanish) and a value record in
    the branch "value clipped and chosen" — v_old = v - 15, vtarg = v + 20 with vf_clip = 10: f2 = 25^2 > f1 = 20^2 and the
    clipped branch is constant — whose gradient is exactly zero and which stays in that branch under any head error far below 1.
    With kl_coeff = ent_coeff = 0 the head gradient of a silent sample is exactly zero."""
    v = np.asarray(heads_v, np.float64)[:, 0]
    out = {k: np.array(val, copy=True) for k, val in rec.items()}
    out["adv"][:] = 0.0
    out["values"] = _f32(v - SILENT_DV)
    out["vtarg"] = _f32(v + SILENT_VT)
    return out


def loud(table):
    """The record in which EVERY sample is loud: a surrogate inside the clip range (ratio target 1.0, advantage +|adv| of the
    table) and an unclipped value step (v - v_old = 3, vtarg - v = 3).  Sample k of it is what one_hot_general puts at k; as
    the loss is a per-sample function (times 1 / B), its head gradient row k is the one-hot batch's."""
    hp, hv, rec = table["head_p"], table["head_v"], table["rec"]
    out = {k: np.array(val, copy=True) for k, val in rec.items()}
    out["logp"] = _f32(lref._logp64(rec["actions"].astype(np.float64), hp[:, :6], np.clip(hp[:, 6:12], -20.0, 2.0)))
    out["adv"] = np.abs(rec["adv"])
    out["values"] = _f32(hv[:, 0] - LOUD_DV)
    out["vtarg"] = _f32(hv[:, 0] + LOUD_VT)
    return out


def one_hot_general(table, k):
    """The table's batch with every sample silenced except sample k, which carries its loud row."""
    rec, hot = silence(table["rec"], table["head_v"]), loud(table)
    for key in lref.REC_KEYS:
        rec[key][k] = hot[key][k]
    return rec


def check_conditions_general(head_p, head_v, rec):
    """ppo_loss_ref.check_conditions, and — the heads are a net's, not a chosen row — no raw log-std within 0.05 of the clamp's bounds."""
    raw = np.asarray(head_p, np.float64)[:, 6:12]
    assert np.all(np.abs(raw - 2.0) >= 0.05) and np.all(np.abs(raw + 20.0) >= 0.05)
    return lref.check_conditions(head_p, head_v, rec)
