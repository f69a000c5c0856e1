"""tests/mlp_grad_ref.py — the float64 reference the weight-gradient kernels are held against element by element
(test_gpu_mlp_wgrad.py) — against float64 torch autograd of the module itself, its reading of the stored operand planes against a
CPU statement of the split, its silent and loud record rows against tests/ppo_loss_ref.py, and the slicing its batch sizes are
chosen from against the table of the GPU test."""
import numpy as np
import pytest
import torch

import mlp_grad_ref as ref
import ppo_loss_ref as lref

BATCHES = (1, 17, 33, 63, 64, 97, 130, 2113, 4177)        # the GPU test's


def _model(seed):
    """gpu_support.mlp_make's model on the CPU: heads of visible size, non-zero biases"""
    from pioneer_amd.ppo import ActorCritic, PPOConfig
    torch.manual_seed(seed)
    model = ActorCritic(PPOConfig())
    with torch.no_grad():
        for net in (model.policy, model.value):
            for l in net:
                if isinstance(l, torch.nn.Linear):
                    l.bias.normal_(0, 0.1)
        model.policy[4].weight.mul_(30.0)
    return model


def _inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.clamp((torch.randn(B, 137, generator=g) * 2.0 + 0.3 - 0.2) * 0.8, min=-2.5, max=2.5)
    g_head = torch.randn(2, B, 16, generator=g) / B
    g_head[0, :, 12:] = 0
    g_head[1, :, 1:] = 0
    return x, g_head


@pytest.mark.parametrize("B", [1, 5, 67])
def test_backward_ref_equals_float64_autograd(B):
    model = _model(B)
    x, g_head = _inputs(B, B + 1)
    nets = ref.backward_ref(model, x, g_head, None)
    m64 = _model(B).double()
    x64 = x.double()
    for n, (net, want) in enumerate(zip((m64.policy, m64.value), nets)):
        lins = [l for l in net if isinstance(l, torch.nn.Linear)]
        h1 = torch.tanh(lins[0](x64)); h1.retain_grad()
        h2 = torch.tanh(lins[1](h1)); h2.retain_grad()
        head = lins[2](h2)
        n3 = head.shape[1]
        (head * g_head[n, :, :n3].double()).sum().backward()
        close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1e-300)   # noqa: E731
        assert close(want["h1"], h1.detach()) and close(want["h2"], h2.detach())
        assert close(want["head"][:, :n3], head.detach()) and not want["head"][:, n3:].any()
        assert close(want["dz2"], (h2.grad * (1 - h2 * h2)).detach()) and close(want["dz1"], (h1.grad * (1 - h1 * h1)).detach())
        params = [t for l in lins for t in (l.weight, l.bias)]
        for got, prm in zip(want["grads"], params):
            assert got.shape == prm.grad.shape and close(got, prm.grad)
        # every entry is below its sum of absolute terms
        assert bool((want["dz2"].abs() <= want["abs"]["dz2"] * (1 + 1e-12)).all()) and bool((want["dz1"].abs() <= want["abs"]["dz1"] * (1 + 1e-12)).all())
        assert bool((want["h1"].abs() <= want["abs"]["h1"]).all()) and bool((want["h2"].abs() <= want["abs"]["h2"]).all())


def test_bf16_rounding_points_and_emulate():
    """rounding = "bf16": every stored tensor is a bf16 number, and emulate() is that chain's heads and gradients."""
    model = _model(3)
    x, g_head = _inputs(33, 4)
    nets = ref.backward_ref(model, x, g_head, "bf16")
    for net in nets:
        for k in ("x", "h1", "h2", "g", "dz2", "dz1"):
            assert torch.equal(net[k], ref.bf(net[k])), k
    heads, grads = ref.emulate(model, x, g_head)
    assert torch.equal(heads, torch.stack([n["head"] for n in nets])) and len(grads) == 12
    assert all(torch.equal(a, b) for a, b in zip(grads, [g for n in nets for g in n["grads"]]))
    plain = ref.backward_ref(model, x, g_head, None)
    for a, b in zip(nets, plain):      # bf16 operands cost a few 1e-3 of the gradients, not more
        for ga, gb in zip(a["grads"], b["grads"]):
            assert float((ga - gb).norm() / gb.norm()) < 3e-2


def test_gemm_ref_is_the_product_and_its_sum_of_absolute_terms():
    g = torch.Generator().manual_seed(1)
    a, b = torch.randn(37, 5, generator=g), torch.randn(37, 3, generator=g)
    p, s = ref.gemm_ref(a, b)
    want = sum(torch.outer(a[i].double(), b[i].double()) for i in range(37))
    wabs = sum(torch.outer(a[i].double().abs(), b[i].double().abs()) for i in range(37))
    assert float((p - want).abs().max()) <= 1e-14 and float((s - wabs).abs().max()) <= 1e-14 and bool((p.abs() <= s + 1e-14).all())


@pytest.mark.parametrize("kind,B,scale", [("act", 130, 1.0), ("input", 130, 2.5), ("grad", 130, 1.0 / 130), ("grad", 4177, 20.0 / 4177)])
def test_planes_round_trip(kind, B, scale):
    """Values split on the CPU as the kernels split them come back: one bf16 plane to 2^-8 (half an ulp), two fp16 planes to 2^-22 (11 + 11
    significant bits; plus half a subnormal step of the residual plane, 2^-25 over the tensor's scale, which is what the scales
    keep small), three bf16 planes exactly — relative to the value."""
    g = torch.Generator().manual_seed(7)
    v = (torch.rand(2, 50, 256, generator=g) * 2 - 1) * scale
    v[0, 0, :4] = torch.tensor([0.0, scale, -scale, scale * 2.0 ** -9])
    for planes, tol in ((1, 2.0 ** -8), (2, 2.0 ** -22), (3, 0.0)):
        buf = ref.split_planes(v, planes, kind, B)
        assert buf.dtype == torch.bfloat16 and tuple(buf.shape) == (planes, 2, 50, 256)
        back = ref.planes_to_f64(buf, planes, kind, B)
        floor = 2.0 ** -25 / {"act": ref.SCALE_ACT, "input": ref.SCALE_INPUT, "grad": ref.grad_scale(B)}[kind] if planes == 2 else 0.0
        assert back.dtype == torch.float64 and bool(((back - v.double()).abs() <= tol * v.double().abs() + floor).all()), planes
    assert ref.grad_scale(1) == 4.0 and ref.grad_scale(130) == 4.0 * 256 and ref.grad_scale(4096) == 4.0 * 4096 and ref.grad_scale(4177) == 4.0 * 8192


def _table(B):
    model = _model(B % 97)
    x, _ = _inputs(B, B + 2)
    nets = ref.backward_ref(model, x, None, None)
    hp, hv = nets[0]["head"].numpy(), nets[1]["head"].numpy()
    return ref.make_table_general(hp, hv, seed=B)


@pytest.mark.parametrize("B", [1, 63, 130, 2113])
def test_record_rows_pass_the_conditions_and_silent_rows_are_exactly_zero(B):
    """Every row the GPU tests use — the dense table, the silent rows and the loud rows around a net's own heads — passes
    ppo_loss_ref.check_conditions; a silent sample's head gradient is exactly zero, a loud one's is not."""
    tab = _table(B)
    hp, hv = tab["head_p"], tab["head_v"]
    r = ref.check_conditions_general(hp, hv, tab["rec"])
    assert np.all(np.abs(r["ratio"] / tab["target"] - 1.0) < 1e-5) and np.all(np.abs(r["dv"] - tab["dv_case"]) < 1e-5)
    silent = ref.silence(tab["rec"], hv)
    ref.check_conditions_general(hp, hv, silent)
    r = lref.ppo_loss_ref(hp, hv, silent, kl_coeff=0.0, ent_coeff=0.0)
    assert not r["g_head"].any()
    br = lref.branches(silent, r)
    assert bool(br["value clipped and chosen"].all())
    everyone = ref.loud(tab)
    ref.check_conditions_general(hp, hv, everyone)
    rl = lref.ppo_loss_ref(hp, hv, everyone, kl_coeff=0.0, ent_coeff=0.0)
    assert bool(rl["inrange"].all()) and np.all(np.abs(rl["ratio"] - 1.0) < 1e-5) and np.all(np.abs(rl["dv"] - ref.LOUD_DV) < 1e-5)
    assert bool(rl["g_head"][0, :, :12].any(1).all()) and bool(np.all(rl["g_head"][1, :, 0] != 0.0))
    for k in sorted({0, B // 2, B - 1}):
        rec = ref.one_hot_general(tab, k)
        ref.check_conditions_general(hp, hv, rec)
        r = lref.ppo_loss_ref(hp, hv, rec, kl_coeff=0.0, ent_coeff=0.0)
        others = np.arange(B) != k
        assert not r["g_head"][:, others].any()
        assert np.array_equal(r["g_head"][:, k], rl["g_head"][:, k])       # the loud record's row k IS the one-hot batch's


def test_batch_sizes_give_the_slices_they_were_chosen_for():
    """(slices, rows per slice, rows of the last slice) of the GPU test's batch sizes."""
    want = {1: (1, 64, 1), 17: (1, 64, 17), 33: (1, 64, 33), 63: (1, 64, 63), 64: (1, 64, 64), 97: (2, 64, 33), 130: (3, 64, 2),
            2113: (17, 128, 65), 4177: (22, 192, 145)}
    assert sorted(want) == sorted(BATCHES)
    for B, (slices, rows, last) in want.items():
        s, r = ref.mlp_slicing(B)
        assert (s, r, B - (s - 1) * r) == (slices, rows, last), B
        assert r % 64 == 0 and (s - 1) * r < B <= s * r
