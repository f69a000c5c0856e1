"""tests/adam_ref.py — the float64 reference mlp_adam_kernel is held against element by element (test_gpu_mlp_adam.py) — against
float64 torch.optim.Adam with the same widened hyperparameters, its table against what the GPU test relies on (every class in
every region, the quads with one live element), and its restatement of the packed weights against the properties of a packing: a
bijection onto the buffer, planes that add up to the float32 value."""
import numpy as np
import pytest
import torch

import adam_ref as ar
import mlp_grad_ref as gref
from gpu_support import unpack_flat

W = lambda x: float(np.float32(x))      # noqa: E731  (a hyperparameter as the C ABI carries it)


def _torch_adam(p0, m0, v0, g, t, lr, betas, eps):
    """one float64 torch.optim.Adam step from the state (t - 1, m0, v0): p, m, v"""
    p = torch.nn.Parameter(torch.from_numpy(np.array(p0, np.float64)))
    opt = torch.optim.Adam([p], lr=lr, betas=betas, eps=eps, foreach=False)
    opt.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.from_numpy(np.array(m0, np.float64)),
                    "exp_avg_sq": torch.from_numpy(np.array(v0, np.float64))}
    p.grad = torch.from_numpy(np.array(g, np.float64))
    opt.step()
    st = opt.state[p]
    assert float(st["step"]) == t
    return p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


def _close(a, b, scale=None):
    scale = np.maximum(np.abs(a), np.abs(b)) if scale is None else scale
    return bool(np.all(np.abs(a - b) <= 1e-12 * scale))


@pytest.mark.parametrize("betas,scale", [((0.9, 0.999), 1.0), ((0.9, 0.999), 1.0 / 3.0), ((0.5, 0.9), 0.125)])
def test_adam_ref_equals_float64_torch_adam_over_five_updates(betas, scale):
    lr, eps = W(1e-3), W(1e-8)
    wb = (W(betas[0]), W(betas[1]))
    tab = ar.adam_table(0)
    rng = np.random.RandomState(1)
    p = rng.normal(0.0, 0.06, size=(2, ar.E))
    m, v = tab["m0"].astype(np.float64), tab["v0"].astype(np.float64)
    tp, tm, tv = p.copy(), m.copy(), v.copy()
    sm, sp = np.zeros_like(p), np.zeros_like(p)
    for t in range(1, 6):
        g = ar.adam_table(t - 1)["g"]
        gs = ar.f32(g.astype(np.float64) * W(scale))               # what the kernel multiplies out
        got = ar.adam_ref(p, m, v, g, scale, t, 1e-3, betas, 1e-8)
        assert np.array_equal(got["g"], gs)
        # (a) ONE step from the same state.  m may cancel — the opposing class does — so its error, and the step's, are relative
        # to the terms, |m0| + |g'|.  The step itself, free of p's own size: a parameter at zero comes out as -d
        absm = np.abs(m) + np.abs(gs)
        absd = got["lr1"] * absm / got["denom"]
        zp, zm, zv = _torch_adam(np.zeros_like(p), m, v, gs, t, lr, wb, eps)
        assert _close(got["d"], -zp, absd) and np.array_equal(got["p"], p - got["d"])
        assert _close(got["m"], zm, absm) and _close(got["v"], zv)
        # (b) the two chains, each on its own state: what an element's m lost to a cancellation in an earlier step stays in it, so
        # the terms add up along the chain
        tp, tm, tv = _torch_adam(tp, tm, tv, gs, t, lr, wb, eps)
        p, m, v = got["p"], got["m"], got["v"]
        sm += absm
        sp += got["lr1"] * sm / got["denom"]
        assert _close(p, tp, np.abs(p) + sp) and _close(m, tm, sm) and _close(v, tv)
    near_eps = np.isin(tab["mag"], (1, 2, 3)) & (tab["region"] != ar.PADDING)
    assert near_eps.sum() > 50000                                  # the classes at and below eps took part


def test_the_step_is_sensitive_to_where_eps_sits():
    """what the table's small gradients are for: eps inside the division by sqrt(1 - b2^t) is a 31-fold larger eps at t = 1"""
    g = np.float32(1e-12)
    r = ar.adam_ref(0.0, 0.0, 0.0, g, 1.0, 1, 1e-3, (0.9, 0.999), 1e-8)
    bc2 = 1.0 - W(0.999)
    moved = W(1e-3) / (1.0 - W(0.9)) * r["m"] / ((np.sqrt(r["v"]) + W(1e-8)) / np.sqrt(bc2))
    assert 25.0 < r["d"] / moved < 35.0 and abs(r["d"] - moved) > 1e4 * r["bound_d"]


def test_every_bound_is_finite_and_positive_where_the_value_can_be_non_zero():
    rng = np.random.RandomState(2)
    p0 = rng.normal(0.0, 0.06, size=(2, ar.E)).astype(np.float32)
    for seed, t, scale, betas in ((0, 1, 1.0, (0.9, 0.999)), (1, 2, 0.5, (0.5, 0.9)), (2, 1000, 1.0 / 3.0, (0.9, 0.999)), (3, 100000, 0.125, (0.9, 0.999))):
        tab = ar.adam_table(seed)
        r = ar.adam_ref(p0, tab["m0"], tab["v0"], tab["g"], scale, t, 1e-3, betas, 1e-8)
        for k, x in r.items():
            assert np.all(np.isfinite(x)), k
        terms = np.abs(tab["m0"].astype(np.float64)) + np.abs(r["g"])
        assert np.all((r["bound_m"] > 0) == (terms > 0)) and np.all(np.abs(r["m"]) <= terms)
        assert np.all((r["bound_v"] > 0) == (r["v"] > 0))
        assert np.all(r["bound_d"][(r["d"] != 0) | (terms > 0)] > 0) and np.all(r["bound_p"][(r["p"] != 0) | (terms > 0)] > 0)
        assert np.all(r["bound_p"] >= r["bound_d"])
        # a one-step bound: a few float32 roundings of the quantity's own terms, not more
        assert np.all(r["bound_m"] <= 4 * ar.U * terms) and np.all(r["bound_v"] <= 4 * ar.U * r["v"])


def test_powf_terms_of_the_step_bound():
    """the bias corrections' share of bound_d: 2^-24 / 0.1 + 2^-24 / (2 * 0.001) at t = 1, nothing at t = 100 000"""
    one = dict(p0=0.0, m0=0.0, v0=0.0, g=np.float32(1.0), scale=1.0, lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    first, late = ar.adam_ref(t=1, **one), ar.adam_ref(t=100000, **one)
    rel = lambda r: float(r["bound_d"] / abs(r["d"]))      # noqa: E731
    pw = ar.K_POW * (ar.U / (1.0 - W(0.9)) + ar.U / (2.0 * (1.0 - W(0.999))))
    assert abs(rel(first) - rel(late) - pw) <= 1e-3 * pw
    assert float(ar.ulp32(0.9)) == 2.0 ** -24 and float(ar.ulp32(1.0)) == 2.0 ** -23 and float(ar.ulp32(0.0)) == 2.0 ** -149


def test_table_holds_every_class_in_every_region_and_the_one_live_element_quads():
    union_b3 = set()
    for seed in ar.TABLE_SEEDS:
        tab = ar.adam_table(seed)
        again = ar.adam_table(seed)
        assert all(np.array_equal(tab[k], again[k]) for k in tab)                   # deterministic
        region, mag, sign, state = tab["region"], tab["mag"], tab["sign"], tab["state"]
        g, m0, v0 = (tab[k].astype(np.float64) for k in ("g", "m0", "v0"))
        assert tab["g"].dtype == np.float32 and tab["g"].shape == (2, ar.E)
        for r in range(5):                                                          # W1, W2, W3, b1, b2: every triple, either sign
            for n in range(2):
                sel = region[n] == r
                combos = set(zip(mag[n, sel].tolist(), sign[n, sel].tolist(), state[n, sel].tolist()))
                assert len(combos) == ar.N_COMBOS, (seed, ar.REGIONS[r], n, len(combos))
        sel = region == 5
        assert int(sel.sum()) == 13
        union_b3 |= set(zip(mag[sel].tolist(), sign[sel].tolist(), state[sel].tolist()))
        # the classes are what they say
        want = np.asarray(ar.G_MAGS)[mag]
        assert np.all((np.abs(g) >= want * (1 - 1e-6)) & (np.abs(g) <= 1.25 * want * (1 + 1e-6))) and np.all((g < 0) <= (sign == 1))
        assert not np.any(m0[state == 0]) and not np.any(v0[state == 0])
        assert np.array_equal(tab["m0"][state == 2], -tab["g"][state == 2])
        stale = (state == 3) & (mag > 0)
        assert np.all(np.abs(v0[stale] / (1e4 * g[stale] ** 2) - 1.0) < 1e-6)
        warm = (state == 1) & (mag > 0)
        assert np.all((m0[warm] / g[warm] > 0.49) & (m0[warm] / g[warm] < 1.51) & (v0[warm] / g[warm] ** 2 > 0.49) & (v0[warm] / g[warm] ** 2 < 1.51))
        # padding: non-zero everywhere
        pad = region == ar.PADDING
        assert np.all(g[pad] != 0) and np.all(m0[pad] != 0) and np.all(v0[pad] != 0)
        # the quads of a thread (four consecutive elements) mix classes: hardly any quad of W2 is of one class
        q = (mag[0, ar.G_W2:ar.G_W3].astype(np.int64) * 4 + state[0, ar.G_W2:ar.G_W3]).reshape(-1, 4)
        assert np.mean((q == q[:, :1]).all(1)) < 0.01
        # every W1 row-end quad holds one live element and three of padding; so does the value net's first b3 quad
        w1 = region[:, :ar.G_W2].reshape(2, 256, 144)
        assert np.all(w1[:, :, 136] == 0) and np.all(w1[:, :, 137:] == ar.PADDING) and np.all(w1[:, :, :137] == 0)
        assert int((g[:, :ar.G_W2].reshape(2, 256, 144)[:, :, 136] != 0).sum()) >= 400      # .. most of them with a gradient
        assert region[1, ar.G_B3] == 5 and np.all(region[1, ar.G_B3 + 1:] == ar.PADDING)
        assert np.all(region[0, ar.G_B3:ar.G_B3 + 12] == 5) and np.all(region[0, ar.G_B3 + 12:] == ar.PADDING)
        assert np.all(region[0, ar.G_W3:ar.G_W3 + 12 * 256] == 2) and np.all(region[0, ar.G_W3 + 12 * 256:ar.G_B1] == ar.PADDING)
        assert np.all(region[1, ar.G_W3:ar.G_W3 + 256] == 2) and np.all(region[1, ar.G_W3 + 256:ar.G_B1] == ar.PADDING)
    assert len(union_b3) == ar.N_COMBOS                                             # b3: over the seeds the GPU test uses


def test_regions_are_unpack_flat_s_layout():
    """a bucket whose entries are their region labels, read through gpu_support.unpack_flat: every tensor sees its own label only,
    and everything unpack_flat leaves out is padding"""
    region = ar.regions()
    flat = torch.from_numpy(region.astype(np.float32).ravel().copy())
    seen = torch.zeros_like(flat)
    marks = torch.zeros_like(flat)
    views = unpack_flat(flat)
    for k, t in enumerate(views):
        label = (0, 3, 1, 4, 2, 5)[k % 6]                     # W1, b1, W2, b2, W3, b3
        assert bool((t == label).all()), k
    for t in unpack_flat(marks):
        t += 1.0
    assert bool(((marks == 1) == (flat != ar.PADDING)).all()) and float(marks.max()) == 1.0
    assert seen.numel() == 2 * ar.E


def _params(seed):
    rng = np.random.RandomState(seed)
    shapes = []
    for n3 in ar.N3:
        shapes += [(256, 137), (256,), (256, 256), (256,), (n3, 256), (n3,)]
    out = [torch.from_numpy((rng.normal(size=s) * 10.0 ** rng.uniform(-6, 1, size=s)).astype(np.float32)) for s in shapes]
    out[0][0, 0], out[0][0, 1], out[2][0, 0] = 0.0, 2.0 ** -30, -3.0           # a zero, a weight whose second fp16 plane is subnormal
    return out


def test_pack_ref_is_a_bijection_that_puts_every_weight_where_the_offsets_say():
    idx = ar.pack_index()
    every = np.concatenate([v.ravel() for v in idx.values()])
    assert np.array_equal(np.sort(every), np.arange(ar.PACK_ELEMS))
    assert [int(idx[k].min()) for k in ("W1", "W2", "W3", "W2T", "W3T")] == [ar.OFF_W1, ar.OFF_W2, ar.OFF_W3, ar.OFF_W2T, ar.OFF_W3T]
    assert int(idx["W3T"].max()) == ar.PACK_ELEMS - 1 == 176127
    # a fragment's eight consecutive k are contiguous, and a 32 x 16 block is 512 elements of its own
    assert np.all(np.diff(idx["W2"].reshape(256, 32, 8), axis=2) == 1)
    assert np.array_equal(np.sort(idx["W2"][:32, :16].ravel()), ar.OFF_W2 + np.arange(512))
    assert np.array_equal(np.sort(idx["W3"][:, :32].ravel()), ar.OFF_W3 + np.arange(512))
    params = _params(3)
    wp, bias = ar.pack_ref(params, ar.N3, 1)
    assert wp.dtype == torch.bfloat16 and tuple(wp.shape) == (1, 2, ar.PACK_ELEMS) and tuple(bias.shape) == (2, ar.BIAS_ELEMS)
    for n in range(2):
        w1, b1, w2, b2, w3, b3 = params[6 * n:6 * n + 6]
        got = wp[0, n]
        bf = lambda t: t.to(torch.bfloat16)      # noqa: E731
        assert torch.equal(got[torch.from_numpy(idx["W1"][:, :137])], bf(w1)) and not got[torch.from_numpy(idx["W1"][:, 137:])].any()
        assert torch.equal(got[torch.from_numpy(idx["W2"])], bf(w2)) and torch.equal(got[torch.from_numpy(idx["W2T"])], bf(w2.t()))
        n3 = ar.N3[n]
        assert torch.equal(got[torch.from_numpy(idx["W3"][:n3])], bf(w3)) and not got[torch.from_numpy(idx["W3"][n3:])].any()
        assert torch.equal(got[torch.from_numpy(idx["W3T"][:, :n3])], bf(w3.t())) and not got[torch.from_numpy(idx["W3T"][:, n3:])].any()
        assert torch.equal(bias[n, :256], b1) and torch.equal(bias[n, 256:512], b2) and torch.equal(bias[n, 512:512 + n3], b3)
        assert not bias[n, 512 + n3:].any()


@pytest.mark.parametrize("planes", [2, 3])
def test_pack_ref_planes_add_up_to_the_float32_weight(planes):
    params = _params(4)
    one, _ = ar.pack_ref(params, ar.N3, 1)
    wp, _ = ar.pack_ref(params, ar.N3, planes)
    assert tuple(wp.shape) == (planes, 2, ar.PACK_ELEMS)
    idx = ar.pack_index()
    tot = gref.planes_to_f64(wp, planes, "weight", 0)
    for n in range(2):
        w1, _, w2, _, w3, _ = params[6 * n:6 * n + 6]
        for name, w in (("W1", torch.cat([w1, torch.zeros(256, 7)], 1)), ("W2", w2), ("W2T", w2.t()),
                        ("W3", torch.cat([w3, torch.zeros(16 - ar.N3[n], 256)])), ("W3T", torch.cat([w3, torch.zeros(16 - ar.N3[n], 256)]).t())):
            got, want = tot[n][torch.from_numpy(idx[name])], w.double()
            if planes == 3:
                assert torch.equal(got, want), name
            else:       # two fp16 planes of 256 w: 2^-22 relative, and the second plane's subnormal spacing 2^-24 (half of it, over 256)
                assert bool(((got - want).abs() <= 2.0 ** -22 * want.abs() + 2.0 ** -33).all()), name
    if planes == 3:
        assert torch.equal(wp[0], one[0])
