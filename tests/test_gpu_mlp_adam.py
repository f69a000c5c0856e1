"""mlp_adam_kernel (csrc/pnr_mlp_adam.h: the slab sum, Adam on the float32 masters, m and v, the re-pack of every 16-bit weight plane
with its transposed copies, the bias copy) ELEMENT BY ELEMENT against tests/adam_ref.py — float64 Adam with a derived bound per
element (the derivation is that module's docstring; tests/test_adam_ref_cpu.py holds it against float64 torch.optim.Adam) and a CPU
restatement of the packed planes.

The model's twelve parameter tensors live in ONE sentinel-filled arena, 64 floats of guard band on both sides of each, so a store
beside a tensor — the W1 row ends, where a thread's quad holds one live element, the W3 rows and b3 entries >= n3, the value net's
one live b3 float — shows.  m and v are filled from adam_ref.adam_table: every (gradient class, state class) in every region,
gradients at and below eps, and non-zero g, m, v on the padding, which the kernel must leave alone.

(a) one update, every element: p, m, v of every live element within adam_ref's bounds; padding m, v and the arena's guards bit-intact;
    every plane of wpack, and bias, bit-equal to pack_ref of the UPDATED masters — and a plain pnr_mlp_pack of the same masters too.
(b) eight consecutive updates, the reference re-based on the kernel's own float32 state after each: one-step bounds throughout.
(c) net selection, nets in {None, (0, 1), (1, 1)}: the selected net as the both-nets call leaves it, the other net untouched, the
    value net's chain on its own update counter.
(d) the slab sum's three paths (a batch of 32, blocks of 8, singles) at slice counts 7, 8, 9, 17, 31: the fused reduce + Adam form
    equals the flat-bucket form bit for bit — which (a) ties to float64 —, and a one-net train_step writes its half of the bucket only.

The worst err / bound ratios go to mlp_adam_margins.json (test_gpu_dynamics._record_margin)."""
import functools

import numpy as np
import pytest
import torch

import adam_ref as ar
import mlp_grad_ref as gref
from gpu_support import mlp_make as make, unpack_flat

pytestmark = pytest.mark.gpu
SENTINEL = -777.25
GUARD = 64
LR, EPS = 1e-3, 1e-8
E, N3 = ar.E, ar.N3
BETAS, OTHER_BETAS = (0.9, 0.999), (0.5, 0.9)
THIRD = 1.0 / 3.0


def _record_margin(case, figures):
    from test_gpu_dynamics import _record_margin as record
    print(f"mlp adam [{case}]: {figures}")
    record(case, None, None, file="mlp_adam_margins.json", figures=figures)


def _ratio(err, bound):
    """the worst err / bound; where the bound is zero the error must be"""
    safe = np.where(bound > 0, bound, 1.0)
    r = np.where(bound > 0, err / safe, np.where(err == 0, 0.0, np.inf))
    return float(r.max())


def _np(t):
    return t.detach().cpu().numpy()


def _u32(t):
    return _np(t.contiguous()).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _table(seed):
    return ar.adam_table(seed)


class _Rig:
    """a model whose parameters live in one guarded arena, and its HipMLP"""

    def __init__(self, planes, seed=5):
        from pioneer_amd.mlp import HipMLP
        model, _, obs, _, _ = make(64, seed=seed)
        self.dev = dev = obs.device
        params = [t for net in (model.policy, model.value) for l in net if isinstance(l, torch.nn.Linear) for t in (l.weight, l.bias)]
        self.init = [p.detach().clone() for p in params]
        pad4 = lambda n: (n + 3) // 4 * 4      # noqa: E731
        self.arena = torch.full((sum(pad4(p.numel()) + GUARD for p in params) + GUARD,), SENTINEL, device=dev)
        self.guard = torch.ones(self.arena.numel(), dtype=torch.bool, device=dev)
        o = GUARD
        for p in params:
            n = p.numel()
            assert o % 4 == 0
            p.data = self.arena[o:o + n].view(p.shape)
            self.guard[o:o + n] = False
            o += pad4(n) + GUARD
        assert o == self.arena.numel() and self.arena.data_ptr() % 16 == 0
        self.mlp = HipMLP(model, 64, dev, planes=planes)
        assert [p.data_ptr() for p in self.mlp.params] == [p.data_ptr() for p in params]
        self.planes = planes
        self.m, self.v, self.step = self.mlp.adam_state()

    def reset(self, m0, v0, t, value_t=None):
        """the initial parameters, the given m, v [2, E] and update count(s); sentinels in the packed weights and the bias copy"""
        for p, q in zip(self.mlp.params, self.init):
            p.data.copy_(q)
        self.m.copy_(torch.from_numpy(np.ascontiguousarray(m0)).reshape(-1))
        self.v.copy_(torch.from_numpy(np.ascontiguousarray(v0)).reshape(-1))
        self.step.fill_(float(t if value_t is None else value_t))
        self.mlp.sync_step_counters(True)               # the value net's own count := the common one
        self.step.fill_(float(t))
        self.mlp.wpack.fill_(SENTINEL)
        self.mlp.bias.fill_(SENTINEL)

    def bucket(self):
        """the parameters in the padded bucket layout [2, E], padding zero, as float32 numpy"""
        flat = torch.zeros(2 * E, device=self.dev)
        for view, p in zip(unpack_flat(flat), self.mlp.params):
            view.copy_(p.detach())
        return _np(flat).reshape(2, E)

    def guards_intact(self):
        return bool((self.arena[self.guard] == SENTINEL).all())

    def snapshot(self):
        mlp = self.mlp
        return {"params": [p.detach().clone() for p in mlp.params], "m": self.m.clone().view(2, E), "v": self.v.clone().view(2, E),
                "wpack": mlp.wpack.clone().view(self.planes, 2, ar.PACK_ELEMS), "bias": mlp.bias.clone().view(2, ar.BIAS_ELEMS),
                "step": float(self.step), "step_value": float(mlp._step_value_net)}

    def pack_equals_ref(self):
        """(wpack == pack_ref, bias == pack_ref) of the CURRENT masters, bit for bit"""
        want_w, want_b = ar.pack_ref([p.detach() for p in self.mlp.params], N3, self.planes)
        got_w = self.mlp.wpack.cpu().view(self.planes, 2, ar.PACK_ELEMS)
        return torch.equal(got_w.view(torch.int16), want_w.view(torch.int16)), np.array_equal(_u32(self.mlp.bias), want_b.numpy().view(np.uint32).ravel())


@functools.lru_cache(maxsize=None)
def _rig(planes):
    return _Rig(planes)


def _net_parts(snap, n):
    """everything of net n in a snapshot, as a list of tensors"""
    return snap["params"][6 * n:6 * n + 6] + [snap["m"][n], snap["v"][n], snap["wpack"][:, n], snap["bias"][n]]


def _same_bits(a, b):
    return all(torch.equal(x.contiguous().view(torch.int16), y.contiguous().view(torch.int16)) for x, y in zip(a, b))


def _against_ref(rig, tab_region, p0, m0, v0, g, scale, t, betas, nets=(0, 1)):
    """the worst err / bound of p, m, v over EVERY live element of the given nets, and whether the padding's m and v kept their bits"""
    want = ar.adam_ref(p0, m0, v0, g, scale, t, LR, betas, EPS)
    got = {"p": rig.bucket(), "m": _np(rig.m).reshape(2, E), "v": _np(rig.v).reshape(2, E)}
    nets = list(nets)
    live = tab_region[nets] != ar.PADDING
    fig = {}
    for k in ("p", "m", "v"):
        assert np.all(np.isfinite(got[k]))
        err = np.abs(got[k][nets].astype(np.float64) - want[k][nets])
        fig[k] = _ratio(err[live], want["bound_" + k][nets][live])
    pad = ~live
    kept = all(np.array_equal(got[k][nets].view(np.uint32)[pad], np.asarray(x0, np.float32)[nets].view(np.uint32)[pad]) for k, x0 in (("m", m0), ("v", v0)))
    assert int(live.sum()) + int(pad.sum()) == len(nets) * E and int(pad.sum()) > 0 and int(live.sum()) > 100000 * len(nets)
    return fig, kept, got


# ---- (a) one update, every element ------------------------------------------------------------------------------------------------------
# every t x {1, 1 / 3} at planes = 1; every scale, planes and pair of betas at least once; the table's five seeds all occur
CASES = [(t, s, 1, BETAS) for t in (1, 2, 10, 1000, 100000) for s in (1.0, THIRD)] + [
    (1, 0.5, 2, BETAS), (10, 0.125, 3, OTHER_BETAS), (2, 0.5, 3, BETAS), (1000, 0.125, 2, OTHER_BETAS), (1, 1.0, 1, OTHER_BETAS), (100000, THIRD, 2, BETAS)]


@pytest.mark.parametrize("k", range(len(CASES)), ids=[f"t{t}-scale{s:.3g}-planes{pl}-b{b[0]}" for t, s, pl, b in CASES])
def test_one_update_every_element(k):
    t, scale, planes, betas = CASES[k]
    seed = ar.TABLE_SEEDS[k % len(ar.TABLE_SEEDS)]
    rig, tab = _rig(planes), _table(seed)
    mlp = rig.mlp
    rig.reset(tab["m0"], tab["v0"], t)
    p0 = rig.bucket()
    flat = torch.from_numpy(tab["g"]).to(rig.dev).reshape(-1).contiguous()
    flat0 = flat.clone()
    mlp.adam(flat, scale, LR, betas, EPS)
    torch.cuda.synchronize()
    fig, padding_kept, _ = _against_ref(rig, tab["region"], p0, tab["m0"], tab["v0"], tab["g"], scale, t, betas)
    checks = {"padding_m_v_kept": padding_kept, "guards_intact": rig.guards_intact(), "gradient_untouched": torch.equal(flat.view(torch.int32), flat0.view(torch.int32)),
              "count_untouched": float(rig.step) == float(t)}
    checks["adam_wpack"], checks["adam_bias"] = rig.pack_equals_ref()
    mlp.wpack.fill_(SENTINEL); mlp.bias.fill_(SENTINEL)
    mlp.pack()                                          # the pack kernel itself on the same masters
    torch.cuda.synchronize()
    checks["pack_wpack"], checks["pack_bias"] = rig.pack_equals_ref()
    checks["guards_after_pack"] = rig.guards_intact()
    _record_margin(f"one_update/t{t}/scale{scale:.4g}/planes{planes}/betas{betas[0]}_{betas[1]}/seed{seed}", dict(fig, **checks, bound="adam_ref: C_M 3, C_V 3, C_D 9, K_POW 1"))
    bad = {k_: v_ for k_, v_ in fig.items() if not v_ <= 1.0}
    assert not bad and all(checks.values()), (bad, checks)


# ---- (b) consecutive updates ---------------------------------------------------------------------------------------------------------
def test_eight_consecutive_updates_each_within_the_one_step_bounds():
    rig, tab = _rig(1), _table(0)
    rig.reset(tab["m0"], tab["v0"], 1)
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    kept = True
    p0, m0, v0 = rig.bucket(), tab["m0"], tab["v0"]
    for t in range(1, 9):
        g = ar.adam_table(100 + t)["g"]
        rig.step.fill_(float(t))
        rig.mlp.adam(torch.from_numpy(g).to(rig.dev).reshape(-1).contiguous(), 1.0, LR, BETAS, EPS)
        torch.cuda.synchronize()
        fig, k, got = _against_ref(rig, tab["region"], p0, m0, v0, g, 1.0, t, BETAS)
        worst = {q: max(worst[q], fig[q]) for q in worst}
        kept = kept and k
        p0, m0, v0 = got["p"], got["m"], got["v"]             # re-based on the kernel's own float32 state
    ok_w, ok_b = rig.pack_equals_ref()
    checks = {"padding_m_v_kept": kept, "guards_intact": rig.guards_intact(), "wpack": ok_w, "bias": ok_b}
    _record_margin("eight_updates", dict(worst, **checks))
    assert all(v <= 1.0 for v in worst.values()) and all(checks.values()), (worst, checks)


# ---- (c) net selection ---------------------------------------------------------------------------------------------------------------
NET_PLANES = 2
COMMON_T, VALUE_T = 3, 7


def _net_run(nets, t, value_t, seed=1):
    rig, tab = _rig(NET_PLANES), _table(seed)
    rig.reset(tab["m0"], tab["v0"], t, value_t)
    before = rig.snapshot()
    flat = torch.from_numpy(tab["g"]).to(rig.dev).reshape(-1).contiguous()
    rig.mlp.adam(flat, 0.5, LR, BETAS, EPS, nets=nets)
    torch.cuda.synchronize()
    return rig, tab, before, rig.snapshot()


@pytest.mark.parametrize("nets", [None, (0, 1), (1, 1)], ids=["both", "policy", "value"])
def test_net_selection(nets):
    if nets is None:
        # the default is the explicit two-net range, on the common counter
        _, _, _, want = _net_run((0, 2), COMMON_T, VALUE_T)
        rig, tab, before, got = _net_run(None, COMMON_T, VALUE_T)
        assert _same_bits(_net_parts(got, 0), _net_parts(want, 0)) and _same_bits(_net_parts(got, 1), _net_parts(want, 1))
        fig, kept, _ = _against_ref(rig, tab["region"], _bucket_of(before), tab["m0"], tab["v0"], tab["g"], 0.5, COMMON_T, BETAS)
        chosen = (0, 1)
    else:
        n, other = nets[0], 1 - nets[0]
        t = VALUE_T if nets == (1, 1) else COMMON_T               # the value net's chain counts in a counter of its own
        _, _, _, both = _net_run(None, t, t)
        rig, tab, before, got = _net_run(nets, COMMON_T, VALUE_T)
        assert _same_bits(_net_parts(got, n), _net_parts(both, n)), "the selected net is not what the both-nets call leaves"
        assert _same_bits(_net_parts(got, other), _net_parts(before, other)), "the other net was touched"
        fig, kept, _ = _against_ref(rig, tab["region"], _bucket_of(before), tab["m0"], tab["v0"], tab["g"], 0.5, t, BETAS, nets=(n,))
        chosen = (n,)
    assert (got["step"], got["step_value"]) == (float(COMMON_T), float(VALUE_T))      # pnr_mlp_adam uses the counts as they stand
    _record_margin(f"net_selection/{nets}", dict(fig, padding_m_v_kept=kept, guards_intact=rig.guards_intact(), nets=str(chosen)))
    assert all(fig[q] <= 1.0 for q in ("p", "m", "v")) and kept and rig.guards_intact(), fig


def _bucket_of(snap):
    flat = torch.zeros(2 * E, device=snap["m"].device)
    for view, p in zip(unpack_flat(flat), snap["params"]):
        view.copy_(p)
    return _np(flat).reshape(2, E)


# ---- (d) the slab sum's three paths -----------------------------------------------------------------------------------------------------
SLICES = {448: 7, 512: 8, 576: 9, 2112: 17, 1984: 31}


def _learner_state(mlp):
    m, v, step = mlp.adam_state()
    return [p.detach() for p in mlp.params] + [m, v, mlp.wpack, mlp.bias]


@pytest.mark.parametrize("B", sorted(SLICES))
def test_fused_reduce_and_adam_equals_the_flat_bucket_form(B):
    import copy
    from pioneer_amd.mlp import HipMLP
    from test_gpu_mlp import _record
    slices = SLICES[B]
    R, lr = 2 * B, 1e-3
    model, mlp, obs, _, filt = make(B, seed=17, rows=R, with_filter=True)
    dev = obs.device
    n_grad = int(mlp.lib.pnr_mlp_grad_floats())
    assert gref.mlp_slicing(B)[0] == slices and int(mlp.lib.pnr_mlp_slab_floats(B)) == slices * n_grad and n_grad == 2 * E
    rec = _record(R, dev)
    klc = torch.tensor(0.2, device=dev); entc = torch.tensor(0.01, device=dev)
    model_f = copy.deepcopy(model); mlp_f = HipMLP(model_f, B, dev)          # the flat-bucket form
    model_n = copy.deepcopy(model); mlp_n = HipMLP(model_n, B, dev)          # one-net calls, nothing updated
    for x in (mlp, mlp_f, mlp_n):
        x.pack()
    perm = torch.randperm(R, generator=torch.Generator(device=dev).manual_seed(3), device=dev).contiguous()
    ga = mlp.gather_epoch(obs, perm, filt, rec)
    means = torch.zeros(2, 8, device=dev); means_f = torch.zeros(2, 8, device=dev)
    flat = torch.full((n_grad,), SENTINEL, device=dev)
    args = (klc, entc, 0.3, 10.0, 1.0)
    for it in range(2):
        s0 = it * B
        mb = {k: ga[k][s0:s0 + B] for k in mlp.REC_KEYS}
        xs = ga["xs"][s0:s0 + B]
        mlp.train_step(None, None, None, mb, *args, means[it], lr, xs_in=xs)
        mlp_f.train_step(None, None, None, mb, *args, means_f[it], lr, flat_grad=flat, xs_in=xs)
        if it == 0 and B in (448, 1984):
            both = flat.clone()
            assert bool(torch.isfinite(both).all()) and bool(both.view(2, E)[0].any()) and bool(both.view(2, E)[1].any())
            mlp_n.train_step(None, None, None, mb, *args, torch.zeros(8, device=dev), lr, flat_grad=torch.empty_like(flat), xs_in=xs)
            count = lambda: (float(mlp_n.adam_state()[2]), float(mlp_n._step_value_net))      # noqa: E731
            assert count() == (1.0, 0.0)
            weights = [t.clone() for t in _learner_state(mlp_n)]
            for net, after in ((0, (2.0, 0.0)), (1, (2.0, 1.0))):
                half = torch.full((n_grad,), SENTINEL, device=dev)
                mlp_n.train_step(None, None, None, mb, *args, torch.zeros(8, device=dev), lr, flat_grad=half, xs_in=xs, nets=(net, 1))
                torch.cuda.synchronize()
                h, b = half.view(2, E), both.view(2, E)
                assert torch.equal(h[net].view(torch.int32), b[net].view(torch.int32)), f"net {net}: not the both-nets call's half"
                assert bool((h[1 - net] == SENTINEL).all()), f"net {net}: the other half was written"
                assert count() == after, (net, count())                                  # only that net's update counter advances
            assert _same_bits(weights, _learner_state(mlp_n))
        mlp_f.adam(flat, 1.0, lr)
    torch.cuda.synchronize()
    assert torch.equal(means, means_f)
    assert float(mlp.adam_state()[2]) == 2.0 and float(mlp_f.adam_state()[2]) == 2.0
    assert bool(mlp.adam_state()[0].any()) and bool(mlp.adam_state()[1].any())
    names = ["w1", "b1", "w2", "b2", "w3", "b3"] * 2 + ["m", "v", "wpack", "bias"]
    for name, a, b in zip(names, _learner_state(mlp), _learner_state(mlp_f)):
        assert torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16)), f"{name}: fused reduce + Adam != flat bucket + pnr_mlp_adam"
