"""The weight-gradient kernels (csrc/pnr_mlp_wgrad.h: mlp_wgrad_kernel<NS>, its direct-to-LDS ring, the hand-staged last chunk,
the register-staged roles 2 and 3, the per-tile layer-3 partials and the slab reductions) ELEMENT BY ELEMENT, at the batch sizes
where a chunk schedule goes wrong, on a model whose W3 is not zero and whose tensors have their usual scale.

Batch sizes (tests/mlp_grad_ref.py mlp_slicing; tests/test_mlp_grad_ref_cpu.py holds the table):
  1, 17, 33, 63   one slice of one partial 64-row chunk (32-row chunks: partial | one whole + 1 | one whole + 31)
  64              one whole chunk (two whole 32-row chunks)          97    one chunk, then 33 rows (one whole 32-row chunk + 1)
  130             two one-chunk slices, then 2 rows
  2113            16 slices of 2 chunks — the ring's look-ahead depth — then 65 rows (1 whole + 1 | 2 whole + 1)
  4177            21 slices of 3 chunks, then 145 rows (2 whole + 17 | 4 whole + 17)

Every test has two stages, so that the weight-gradient kernel is judged on the operands it actually read.

Stage 1 — what the earlier kernels stored (xs, h1, h2 where stored, dz2, dz1, g_head where written) against backward_ref.
  planes = 1: |err| <= 2^-7 x the entry's abs-sum (backward_ref's "abs": the sum of the absolute terms of the expression behind the
    entry — sum |x| |w| + |b| for h1 / h2, sum |g| |w| (1 + h^2) for dz2 / dz1, whose tanh derivative is 1 - h^2; the entry itself
    for xs).  Derivation: the kernel and the reference round the same quantity to bf16, computed in float32 there and in float64
    here (the difference, (K + 2) 2^-24 abs-sum and 1e-7 of tanh, is 2^-17 of a bf16 ulp), so the two roundings agree or are
    neighbours: one ulp, and an ulp of a bf16 number v is at most 2^-7 |v|.  The propagated term: an upstream entry that came out
    one ulp off moves its ONE term of the abs-sum by at most 2^-7 of that term, and an entry is off only when its float32 and
    float64 values straddle a rounding boundary (a fraction ~2^-17 / 2^-8 of them), so in a sum of 12 .. 256 terms of both signs
    it stays inside the slack between |v| and the abs-sum.  Not so in the value net's dz2, a ONE-term product g w (1 - h^2): when
    h is an ulp off (<= 2^-8 below 1), h^2 moves by 2 h ulp(h) <= 2^-6 h^2, and with the entry's own rounding, 2^-7 |g w| (1 - h^2),
    the total is 2^-7 |g w| (1 + h^2) — the abs-sum as defined above.  (With the derivative's own two terms left out of the
    abs-sum the value net's dz2 came to 1.07 of the bound at B = 4177, on exactly such an entry.)
  planes = 2, 3: the project's SPLIT_TOL bound, 1e-5 of the largest entry of the sample's row of the float64 (unrounded) chain.
  g_head (planes = 1, w3_partials off): the loss of the heads that the STORED h2 gives, by the fused-loss test's own bound.
  In a one-hot batch every row but the hot sample's must be exactly 0.0.

Stage 2 — every parameter gradient against gemm_ref of the STORED operands (planes_to_f64), padding included.
  dense: |err| <= c x abs-sum, c = (K + 2) 2^-24 (float32 accumulation of K = B terms, the slabs' sum) + the plane pairs a split
    product leaves out (2^-22 two planes, 2^-23 three).  planes = 1 rounds g_head to bf16 before layer 3's products: so does the
    reference.
  one-hot: every element is ONE product.  planes = 1: equal to float32(dz[s, o]) * float32(h[s, i]) bit for bit (a product of two
    bf16 numbers is exact in float32, everything else added is zero); split operands: |err| <= 2^-21 |dz| |h|.  A dropped sample
    shows as zeros, a doubled one as twice the product, a wrong pairing as another sample's outer product.
  The padded W1 columns 137 .. 143, W3 rows >= n3 and b3 entries >= n3 are exactly zero.

Forms: (a) pnr_mlp_backward through autograd (planes = 1: the dW2 ring, the register-staged roles 2 and 3); (b) train_step on
pre-gathered rows, planes 1, 2, 3, the trainer's default (the dW1 ring halves and the per-tile layer-3 partials); (c) planes = 1
with w3_partials off: the same bits as (b), and g_head and h2 in the workspace for dW3 / db3 / db2; (d) accumulate = 1 with a
device scale.  The worst err / bound ratios go to mlp_wgrad_margins.json (test_gpu_dynamics._record_margin)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import mlp_grad_ref as ref
import ppo_loss_ref as lref
from gpu_support import mlp_make as make

pytestmark = pytest.mark.gpu
BATCHES = (1, 17, 33, 63, 64, 97, 130, 2113, 4177)
SMALL = tuple(B for B in BATCHES if B <= 130)
SENTINEL = -777.25
SPLIT_ROW_TOL, SPLIT_MATRIX_TOL = 1e-5, 1e-4                 # test_gpu_mlp.py's SPLIT_TOL
LEFT_OUT = {1: 0.0, 2: 2.0 ** -22, 3: 2.0 ** -23}            # the plane pairs a split product leaves out
E1, E2, E3 = 256 * 144, 256 * 144 + 256 * 256, 256 * 144 + 256 * 256 + 16 * 256      # the bucket's offsets: W2, W3, b1
N3 = (12, 1)


def _record_margin(case, figures):
    from test_gpu_dynamics import _record_margin as record
    print(f"mlp wgrad [{case}]: {figures}")
    record(case, None, None, file="mlp_wgrad_margins.json", figures=figures)


def _ratio(err, bound):
    """the worst err / bound, on the device; where the bound is zero the error must be"""
    inf = torch.full_like(err, float("inf"))
    return torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), inf)).max()


def _dense_c(planes, B):
    c = (B + 2) * 2.0 ** -24 + LEFT_OUT[planes]
    assert c <= 1e-3
    return c


def _positions(B):
    return sorted({p for p in (0, 15, 16, 31, 32, 63, B - 1) if p < B})


def _views(flat):
    """the padded bucket [2][107 024] as {name: [2, ...]}"""
    f = flat.view(2, -1)
    return {"w1": f[:, :E1].reshape(2, 256, 144), "w2": f[:, E1:E2].reshape(2, 256, 256), "w3": f[:, E2:E3].reshape(2, 16, 256),
            "b1": f[:, E3:E3 + 256], "b2": f[:, E3 + 256:E3 + 512], "b3": f[:, E3 + 512:E3 + 528]}


def _padding_is_zero(v):
    return (not bool(v["w1"][:, :, 137:].any()) and not bool(v["w3"][0, 12:].any()) and not bool(v["w3"][1, 1:].any())
            and not bool(v["b3"][0, 12:].any()) and not bool(v["b3"][1, 1:].any()))


@functools.lru_cache(maxsize=None)
def _case(B):
    """the model, its planes = 1 HipMLP, the observations, the filter and the float32 net input of batch size B"""
    model, mlp, obs, _, filt = make(B, seed=B % 97 + 3, with_filter=True)
    x = torch.clamp((obs - filt[0]) * filt[1], min=filt[2], max=filt[3])
    return model, mlp, obs, filt, x


@functools.lru_cache(maxsize=None)
def _mlp(B, planes):
    from pioneer_amd.mlp import HipMLP
    model, mlp1, obs, _, _ = _case(B)
    mlp = mlp1 if planes == 1 else HipMLP(model, B, obs.device, planes=planes)
    mlp.pack()
    return mlp


def _rounding(planes):
    return "bf16" if planes == 1 else None


@functools.lru_cache(maxsize=None)
def _table(B, planes):
    """the case table around the reference's own heads (bf16-rounded chain for planes = 1, float64 otherwise), conditions checked"""
    model, _, _, _, x = _case(B)
    nets = ref.backward_ref(model, x, None, _rounding(planes))
    tab = ref.make_table_general(nets[0]["head"].cpu().numpy(), nets[1]["head"].cpu().numpy(), seed=B)
    for rec in (tab["rec"], ref.silence(tab["rec"], tab["head_v"]), ref.loud(tab)):
        ref.check_conditions_general(tab["head_p"], tab["head_v"], rec)
    return tab


def _dev(rec, dev):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in rec.items()}


def _stored(mlp, xs, B, rows=None):
    """(X [B, 144], h1, dz1, dz2 [2, B, 256]) as float64 from the workspace and the input planes; rows: one sample's rows only"""
    P, ws = mlp.planes, mlp._workspace()
    xs = xs.reshape(P, B, 144)
    pick = (lambda t: t) if rows is None else (lambda t: t[..., rows, :])
    return (ref.planes_to_f64(pick(xs), P, "input", B), ref.planes_to_f64(pick(ws["h1"]), P, "act", B),
            ref.planes_to_f64(pick(ws["dz1"]), P, "grad", B), ref.planes_to_f64(pick(ws["dz2"]), P, "grad", B))


def _stage1(planes, got, want, absum):
    """the worst err / bound of one stored tensor [.., B, F] against the reference"""
    err = (got - want).abs()
    if planes == 1:
        return _ratio(err, 2.0 ** -7 * absum)
    return _ratio(err, SPLIT_ROW_TOL * want.abs().amax(-1, keepdim=True).expand_as(want))


def _x_padded(nets):
    x = nets[0]["x"]
    return torch.cat([x, torch.zeros(x.shape[0], 7, dtype=x.dtype, device=x.device)], 1)


def _stage1_all(planes, nets, X, h1, dz1, dz2, h2=None, rows=None):
    """stage 1 of (X, h1, dz1, dz2[, h2]) against backward_ref's nets; rows: compare these samples' rows only (got has only them)"""
    pick = (lambda t: t) if rows is None else (lambda t: t[rows])
    fig = {"xs": _stage1(planes, X, pick(_x_padded(nets)), pick(_x_padded(nets)).abs())}
    for name, got in (("h1", h1), ("h2", h2), ("dz2", dz2), ("dz1", dz1)):
        if got is None or (name.startswith("dz") and "dz2" not in nets[0]):
            continue
        fig[name] = torch.stack([_stage1(planes, got[n], pick(nets[n][name]), pick(nets[n]["abs"][name])) for n in range(2)]).max()
    return fig


def _dense_stage2(planes, B, got, X, h1, dz1, dz2, g=None, h2=None):
    """every gradient of the padded bucket views `got` against gemm_ref of the stored operands: {name: worst err / bound}"""
    c = _dense_c(planes, B)
    one = torch.ones(B, 1, dtype=torch.float64, device=X.device)
    fig = {}
    for n in range(2):
        prods = {"w1": ref.gemm_ref(dz1[n], X), "b1": ref.gemm_ref(dz1[n], one), "w2": ref.gemm_ref(dz2[n], h1[n]), "b2": ref.gemm_ref(dz2[n], one)}
        if g is not None:
            prods.update(w3=ref.gemm_ref(g[n], h2[n]), b3=ref.gemm_ref(g[n], one))
        for name, (want, absum) in prods.items():
            gv = got[name][n].double()
            r = _ratio((gv - want.reshape(gv.shape)).abs(), c * absum.reshape(gv.shape))
            fig[name] = r if name not in fig else torch.maximum(fig[name], r)
    return fig


def _finish(case, fig, bound):
    fig = {k: float(v) for k, v in fig.items()}
    _record_margin(case, dict(fig, bound=bound))
    bad = {k: v for k, v in fig.items() if not v <= 1.0}
    assert not bad, (case, bad)


# ---- (a) pnr_mlp_backward through autograd: planes = 1, the dW2 ring and the register-staged roles 2 and 3 ------------------------------
def _head_grads(B, dev):
    g = torch.Generator(device=dev).manual_seed(5)
    g_head = torch.randn(2, B, 16, generator=g, device=dev) * (1.0 / B)
    g_head[0, :, 12:] = 0
    g_head[1, :, 1:] = 0
    return g_head


def _backward(B, g_head):
    """mlp.apply + autograd.grad with g_head: the gradients as padded bucket views, the slabs' padding checked"""
    model, mlp, obs, filt, _ = _case(B)
    hp, hv = mlp.apply(obs, None, filt)
    grads = torch.autograd.grad((hp * g_head[0]).sum() + (hv * g_head[1]).sum(), mlp.params)
    dev = obs.device
    got = {"w1": torch.zeros(2, 256, 144, device=dev), "w2": torch.zeros(2, 256, 256, device=dev), "w3": torch.zeros(2, 16, 256, device=dev),
           "b1": torch.zeros(2, 256, device=dev), "b2": torch.zeros(2, 256, device=dev), "b3": torch.zeros(2, 16, device=dev)}
    for n in range(2):
        w1, b1, w2, b2, w3, b3 = grads[6 * n:6 * n + 6]
        got["w1"][n, :, :137] = w1; got["b1"][n] = b1; got["w2"][n] = w2; got["b2"][n] = b2
        got["w3"][n, :N3[n]] = w3; got["b3"][n, :N3[n]] = b3
    slices, _ = ref.mlp_slicing(B)
    ws = mlp._workspace()
    E = int(mlp.lib.pnr_mlp_grad_floats())
    for s in range(slices):          # what the reduction leaves out of the parameter-shaped gradients
        assert _padding_is_zero(_views(ws["slabs"][s * E:(s + 1) * E])), f"slab {s}: padding not zero"
    return mlp, got


@pytest.mark.parametrize("B", BATCHES)
def test_backward_dense(B):
    model, _, obs, _, x = _case(B)
    g_head = _head_grads(B, obs.device)
    mlp, got = _backward(B, g_head)
    ws = mlp._workspace()
    nets = ref.backward_ref(model, x, g_head, "bf16")
    X, h1, dz1, dz2 = _stored(mlp, ws["xs"], B)
    h2 = ws["h2"].double()
    fig = {"s1_" + k: v for k, v in _stage1_all(1, nets, X, h1, dz1, dz2, h2=h2).items()}
    fig.update(_dense_stage2(1, B, got, X, h1, dz1, dz2, g=ref.bf(g_head), h2=h2))
    _finish(f"backward/dense/B{B}", fig, f"stage 1: 2^-7 abs-sum; stage 2: {_dense_c(1, B):.3e} abs-sum")


@pytest.mark.parametrize("B", SMALL)
def test_backward_one_hot(B):
    """g_head is zero but for one sample's row: every gradient element is that sample's one product, bit for bit."""
    model, _, obs, _, x = _case(B)
    dense = _head_grads(B, obs.device)
    nets = ref.backward_ref(model, x, dense, "bf16")           # row k of it is the one-hot batch's row k
    worst = torch.zeros((), dtype=torch.float64, device=obs.device)
    wrong = torch.zeros((), dtype=torch.int64, device=obs.device)
    for k in _positions(B):
        g_head = torch.zeros_like(dense)
        g_head[:, k] = dense[:, k]
        mlp, got = _backward(B, g_head)
        ws = mlp._workspace()
        others = torch.arange(B, device=obs.device) != k
        for name in ("dz1", "dz2"):
            assert not bool(ws[name][0][:, others].any()), f"hot {k}: {name} of a sample without gradient is not 0.0"
        X, h1, dz1, dz2 = _stored(mlp, ws["xs"], B, rows=k)
        h2, g = ws["h2"][:, k].double(), ref.bf(g_head[:, k])
        for v in _stage1_all(1, nets, X, h1, dz1, dz2, h2=h2, rows=k).values():
            worst = torch.maximum(worst, v)
        want = {"w1": dz1[:, :, None] * X[None, None, :], "b1": dz1, "w2": dz2[:, :, None] * h1[:, None, :], "b2": dz2,
                "w3": g[:, :, None] * h2[:, None, :], "b3": g}
        for name, w in want.items():
            assert bool(w.any()), (k, name)
            wrong += (got[name] != w.float()).sum()            # (the float64 product of two bf16 numbers IS their float32 product)
    wrong = int(wrong)
    _record_margin(f"backward/one_hot/B{B}", {"stage1": float(worst), "elements_not_the_product": wrong, "bound": "stage 1: 2^-7 abs-sum; stage 2: equality"})
    assert float(worst) <= 1.0 and wrong == 0, (float(worst), wrong)


# ---- (b), (c) train_step on pre-gathered rows -----------------------------------------------------------------------------------------
def _coeffs(dev, kl, ent):
    return torch.tensor(kl, device=dev), torch.tensor(ent, device=dev)


def _gathered_xs(mlp, B):
    _, _, obs, filt, _ = _case(B)
    dev = obs.device
    z = {k: torch.zeros((B, 6) if k in ("actions", "mean", "log_std") else (B,), device=dev) for k in mlp.REC_KEYS}
    return mlp.gather_epoch(obs, torch.arange(B, device=dev), filt, z)["xs"]


def _step(mlp, xs, rec, klc, entc, flat, means):
    flat.fill_(float("nan")); means.fill_(float("nan"))
    mlp.train_step(None, None, None, rec, klc, entc, lref.CLIP, lref.VF_CLIP, lref.VF_COEFF, means, 1e-3, flat_grad=flat, xs_in=xs)


@functools.lru_cache(maxsize=None)
def _dense_run(planes, B, w3_partials=True):
    """one train_step on the dense table: the bucket, the means, and copies of what the kernels stored"""
    model, _, obs, _, x = _case(B)
    dev = obs.device
    mlp = _mlp(B, planes)
    mlp.w3_partials = w3_partials
    tab = _table(B, planes)
    ws = mlp._workspace()
    if not w3_partials:
        ws["g"].fill_(SENTINEL); ws["h2"].fill_(SENTINEL)
    xs = _gathered_xs(mlp, B)
    flat = torch.empty(int(mlp.lib.pnr_mlp_grad_floats()), device=dev)
    means = torch.empty(8, device=dev)
    _step(mlp, xs, _dev(tab["rec"], dev), *_coeffs(dev, lref.KL_COEFF, lref.ENT_COEFF), flat, means)
    torch.cuda.synchronize()
    mlp.w3_partials = True
    out = {"flat": flat, "means": means, "stored": _stored(mlp, xs, B)}
    if not w3_partials:
        out.update(g=ws["g"][:2 * B * 16].view(2, B, 16).clone(), h2=ws["h2"].clone())
    return out


@functools.lru_cache(maxsize=None)
def _dense_ref(B, planes):
    """backward_ref fed with ppo_loss_ref at the reference's own heads"""
    model, _, obs, _, x = _case(B)
    tab = _table(B, planes)
    want = lref.ppo_loss_ref(tab["head_p"], tab["head_v"], tab["rec"])
    g = torch.from_numpy(want["g_head"]).to(obs.device)
    return want, ref.backward_ref(model, x, g, _rounding(planes))


@pytest.mark.parametrize("planes", [1, 2, 3])
@pytest.mark.parametrize("B", BATCHES)
def test_train_step_dense(planes, B):
    run = _dense_run(planes, B)
    want, nets = _dense_ref(B, planes)
    X, h1, dz1, dz2 = run["stored"]
    got = _views(run["flat"])
    assert bool(torch.isfinite(run["flat"]).all()) and _padding_is_zero(got)
    fig = {"s1_" + k: v for k, v in _stage1_all(planes, nets, X, h1, dz1, dz2).items()}
    fig.update(_dense_stage2(planes, B, got, X, h1, dz1, dz2))
    if planes > 1:       # g_head stays on the chip: layer 3 against the float64 chain, relative to the matrix's largest entry
        for name, i in (("w3", 4), ("b3", 5)):
            # (_ratio: at B = 1 the table's first value row sits in a clipped branch and the value net's gradients are all 0.0)
            r = [_ratio((got[name][n, :N3[n]].double() - nets[n]["grads"][i]).abs(), (SPLIT_MATRIX_TOL * nets[n]["grads"][i].abs().max()).expand_as(nets[n]["grads"][i]))
                 for n in range(2)]
            fig[name] = torch.stack(r).max()
    _finish(f"train_step/dense/planes{planes}/B{B}", fig,
            f"stage 1: {'2^-7 abs-sum' if planes == 1 else '1e-5 row max'}; stage 2: {_dense_c(planes, B):.3e} abs-sum; w3, b3 (planes > 1): 1e-4 matrix max")


@pytest.mark.parametrize("B", BATCHES)
def test_w3_partials_off_gives_the_same_bits_and_layer_3_from_the_stored_operands(B):
    """(c) planes = 1 with H2 and g_head stored and layer 3 made by the weight-gradient kernel's fourth role: bucket and means equal
    the default mode's bit for bit — which carries this test's verdict on dW3 / db3 / db2 over to it."""
    model, _, obs, _, x = _case(B)
    on, off = _dense_run(1, B), _dense_run(1, B, False)
    assert torch.equal(on["flat"], off["flat"]) and torch.equal(on["means"], off["means"])
    for a, b in zip(on["stored"], off["stored"]):
        assert torch.equal(a, b)
    X, h1, dz1, dz2 = off["stored"]
    h2, g = off["h2"].double(), off["g"]
    _, nets = _dense_ref(B, 1)
    fig = {"s1_h2": torch.stack([_stage1(1, h2[n], nets[n]["h2"], nets[n]["abs"]["h2"]) for n in range(2)]).max()}
    # g_head against the loss of the heads the stored h2 gives (float64 products), by the fused-loss test's per-sample bound
    tab = _table(B, 1)
    heads = [torch.zeros(B, 16, dtype=torch.float64, device=obs.device) for _ in range(2)]
    for n, net in enumerate((model.policy, model.value)):
        W3, b3 = ref.linears(net)[4:]
        heads[n][:, :N3[n]] = h2[n] @ ref.bf(W3).t() + b3.double()
    hp, hv = heads[0].cpu().numpy(), heads[1].cpu().numpy()
    want = ref.check_conditions_general(hp, hv, tab["rec"])
    want = lref.ppo_loss_ref(hp, hv, tab["rec"])
    wg = torch.from_numpy(want["g_head"]).to(obs.device)
    assert not bool(g[0, :, 12:].any()) and not bool(g[1, :, 1:].any())
    fig["s1_g_head"] = _ratio((g.double() - wg).abs(), (2e-4 * wg.abs().amax(-1, keepdim=True) + 1e-9).expand_as(wg))
    fig.update(_dense_stage2(1, B, _views(off["flat"]), X, h1, dz1, dz2, g=ref.bf(g), h2=h2))
    _finish(f"train_step/w3_partials_off/B{B}", fig, f"h2: 2^-7 abs-sum; g_head: 2e-4 row max + 1e-9; stage 2: {_dense_c(1, B):.3e} abs-sum")


def _hot_positions(B):
    if B <= 130:
        return _positions(B)
    slices, rows = ref.mlp_slicing(B)
    return list(range(rows, 2 * rows)) + list(range((slices - 1) * rows, B))        # every sample of slice 1 and of the last slice


@pytest.mark.parametrize("planes", [1, 2, 3])
@pytest.mark.parametrize("B", BATCHES)
def test_train_step_one_hot(planes, B):
    """One sample with a gradient (its loud row), every other exactly silent, kl_coeff = ent_coeff = 0: at every position of the
    last slice and of slice 1 for the two large batches, at the chunk and k-step edges for the small ones."""
    model, _, obs, _, x = _case(B)
    dev = obs.device
    mlp = _mlp(B, planes)
    mlp.w3_partials = True
    tab = _table(B, planes)
    everyone = ref.loud(tab)
    g_loud = lref.ppo_loss_ref(tab["head_p"], tab["head_v"], everyone, kl_coeff=0.0, ent_coeff=0.0)["g_head"]
    nets = ref.backward_ref(model, x, torch.from_numpy(g_loud).to(dev), _rounding(planes))     # row k: the one-hot batch around k
    silent, hot = _dev(ref.silence(tab["rec"], tab["head_v"]), dev), _dev(everyone, dev)
    rec = {k: v.clone() for k, v in silent.items()}
    xs = _gathered_xs(mlp, B)
    flat = torch.empty(int(mlp.lib.pnr_mlp_grad_floats()), device=dev)
    means = torch.empty(8, device=dev)
    klc, entc = _coeffs(dev, 0.0, 0.0)
    ws = mlp._workspace()
    worst1 = torch.zeros((), dtype=torch.float64, device=dev)
    worst2 = torch.zeros((), dtype=torch.float64, device=dev)
    worst3 = torch.zeros((), dtype=torch.float64, device=dev)
    wrong = torch.zeros((), dtype=torch.int64, device=dev)
    stray = torch.zeros((), dtype=torch.int64, device=dev)
    sample = torch.arange(B, device=dev)
    for k in _hot_positions(B):
        for key in mlp.REC_KEYS:
            rec[key][k] = hot[key][k]
        _step(mlp, xs, rec, klc, entc, flat, means)
        for key in mlp.REC_KEYS:
            rec[key][k] = silent[key][k]
        got = _views(flat)
        for name in ("dz1", "dz2"):          # [planes, 2, B, 256]: a non-zero pattern in a row that is not the hot sample's
            stray += ((ws[name] != 0).any(-1) & (sample != k)).sum()
        X, h1, dz1, dz2 = _stored(mlp, xs, B, rows=k)
        for v in _stage1_all(planes, nets, X, h1, dz1, dz2, rows=k).values():
            worst1 = torch.maximum(worst1, v)
        want = {"w1": dz1[:, :, None] * X[None, None, :], "b1": dz1, "w2": dz2[:, :, None] * h1[:, None, :], "b2": dz2}
        for name, w in want.items():
            if planes == 1:
                wrong += (got[name] != w.float()).sum()
            else:
                worst2 = torch.maximum(worst2, _ratio((got[name].double() - w).abs(), 2.0 ** -21 * w.abs()))
        stray += got["w1"][:, :, 137:].count_nonzero() + got["w3"][0, 12:].count_nonzero() + got["w3"][1, 1:].count_nonzero() \
            + got["b3"][0, 12:].count_nonzero() + got["b3"][1, 1:].count_nonzero() + (~torch.isfinite(flat)).sum()
        if planes > 1:       # layer 3 against the float64 chain's one product
            for n in range(2):
                w3 = nets[n]["g"][k, :N3[n], None] * nets[n]["h2"][k][None, :]
                worst3 = torch.maximum(worst3, _ratio((got["w3"][n, :N3[n]].double() - w3).abs(), (SPLIT_MATRIX_TOL * w3.abs().max()).expand_as(w3)))
                b3 = nets[n]["g"][k, :N3[n]]
                worst3 = torch.maximum(worst3, _ratio((got["b3"][n, :N3[n]].double() - b3).abs(), (SPLIT_MATRIX_TOL * b3.abs().max()).expand_as(b3)))
        else:
            stray += (got["w3"][0, :12].count_nonzero() == 0).long() + (got["b3"][1, 0] == 0).long()      # layer 3 did get the hot sample
    fig = {"stage1": float(worst1), "stage2": float(worst2), "layer3": float(worst3), "elements_not_the_product": int(wrong), "stray": int(stray)}
    _record_margin(f"train_step/one_hot/planes{planes}/B{B}", dict(fig, positions=len(_hot_positions(B)),
                   bound="stage 1: " + ("2^-7 abs-sum" if planes == 1 else "1e-5 row max") + "; stage 2: " +
                   ("equality" if planes == 1 else "2^-21 |dz| |h|; w3, b3: 1e-4 matrix max")))
    assert fig["stage1"] <= 1.0 and fig["stage2"] <= 1.0 and fig["layer3"] <= 1.0 and fig["elements_not_the_product"] == 0 and fig["stray"] == 0, fig


# ---- (d) pnr_mlp_backward with accumulate = 1 and a device scale ----------------------------------------------------------------------
def test_backward_accumulates_scaled_gradients_and_writes_nothing_else():
    """prev + scale * g, with g the accumulate = 0 result, to one float32 ulp of that sum (the compiler may contract the
    multiply-add: one rounding, or two — half an ulp of scale g and half an ulp of the sum; prev has g's sign, so the sum is the
    larger of the two and its ulp the larger ulp); nothing behind any gradient tensor."""
    B = 97
    model, mlp, obs, filt, _ = _case(B)
    dev = obs.device
    g_head = _head_grads(B, dev)
    mlp.pack()
    head = torch.empty(2, B, 16, device=dev)
    mlp._launch_forward(B, obs, None, filt, head, save=True)
    ws = mlp._workspace()
    GAP = 64
    sizes = [p.numel() for p in mlp.params]
    store = torch.full((sum(sizes) + GAP * (len(sizes) + 1),), SENTINEL, device=dev)
    grads, guard, o = [], torch.ones_like(store, dtype=torch.bool), GAP
    for p, n in zip(mlp.params, sizes):
        grads.append(store[o:o + n].view(p.shape))
        guard[o:o + n] = False
        o += n + GAP

    def backward(accumulate, scale):
        p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        from pioneer_amd import _lib
        _lib.check(mlp.lib.pnr_mlp_backward(B, p(g_head), p(mlp.wpack), p(ws["xs"]), p(ws["h1"]), p(ws["h2"]), p(ws["dz1"]), p(ws["dz2"]),
                                            p(ws["slabs"]), ws["slabs"].numel(), mlp._ptrs(grads), mlp.n3[0], mlp.n3[1], accumulate,
                                            None if scale is None else p(scale), mlp._stream()))
        torch.cuda.synchronize()

    backward(0, None)
    g = [t.clone() for t in grads]
    assert bool((store[guard] == SENTINEL).all()) and all(bool(t.any()) for t in g)
    gen = torch.Generator(device=dev).manual_seed(11)
    # of the gradients' own size and sign
    prev = [torch.where(t < 0, -1.0, 1.0) * (torch.randn(t.shape, generator=gen, device=dev).abs() + 0.01) * float(t.abs().max()) for t in g]
    for t, q in zip(grads, prev):
        t.copy_(q)
    scale = torch.tensor(0.37, device=dev)
    backward(1, scale)
    assert bool((store[guard] == SENTINEL).all()), "written behind a gradient tensor"
    worst = 0.0
    for t, q, gk in zip(grads, prev, g):
        want = q.double() + scale.double() * gk.double()
        ulp = torch.ldexp(torch.ones_like(want), torch.frexp(want)[1] - 24)        # want = m 2^e, 0.5 <= |m| < 1: float32 spacing 2^(e - 24)
        worst = max(worst, float(_ratio((t.double() - want).abs(), ulp)))
    _record_margin("backward/accumulate/B97", {"err_over_bound": worst, "bound": "one float32 ulp of prev + scale g"})
    assert worst <= 1.0, worst
