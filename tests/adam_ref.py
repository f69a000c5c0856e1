"""A float64 restatement of mlp_adam_kernel (csrc/pnr_mlp_adam.h) — one Adam update of the float32 master parameters, element
by element, with a bound on the kernel's float32 rounding beside every value — the table of gradients and optimiser states the
kernel is run on, and the packed 16-bit weight planes restated on the CPU.  tests/test_gpu_mlp_adam.py holds the kernel against
this module; tests/test_adam_ref_cpu.py holds this module against float64 torch.optim.Adam and against itself.

The update (torch.optim.Adam without weight decay or amsgrad), t the update count including this one:
    g' = float32(g * scale)                     m = m0 + (g' - m0) (1 - b1)          v = b2 v0 + (1 - b2) g' g'
    d  = lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)                      p = p0 - d
lr, b1, b2, eps and scale are the float32 numbers the C ABI carries, widened: the kernel is a valid Adam for those.  g * scale is a
product of two float32 numbers; rounded once from float64 to float32 it is the kernel's own correctly rounded product, so g' is
exact here and costs no tolerance.

The bounds.  u = 2^-24 is the relative error of one correctly rounded float32 operation, gamma(n) = n u / (1 - n u) the usual
bound on n of them in a row.  The kernel's operations are counted unfused; under `#pragma clang fp contract(fast)` a multiply may
fuse with the add behind it, which removes a rounding and is covered.  sqrtf and the divisions count as ONE rounding each: the
library is built without any fast-math flag (pioneer_amd/_lib.py HIPCC_FLAGS), and hipcc's default for both is the correctly
rounded form — the count rests on that compiler default.  1 - b1 and 1 - b2 are exact in float32 for betas in [0.5, 1]
(Sterbenz), which adam_ref asserts; nothing in the table comes near the subnormals (the smallest term is 0.1 * (1e-12 / 8)^2).

  m   three operations: s = g' - m0 (error <= u (|g'| + |m0|)), q = s (1 - b1), m = m0 + q (error <= u |m| <= u A), with
      A = |m0| + (1 - b1)(|g'| + |m0|) the sum of the absolute terms.  The first two errors reach m scaled by (1 - b1), so
      |err m| <= gamma(C_M) A, C_M = 3.
  v   four operations on non-negative terms: b2 v0 | ((1 - b2) g') g' (two) | the sum.  The sum's rounding touches both terms, each
      product's its own term: at most three roundings on any term, and the abs-sum is v itself: |err v| <= gamma(C_V) v, C_V = 3.
  d   its own roundings, as relative errors of d: sqrtf(v) 1, sqrtf(1 - b2^t) 1 and half of the subtraction's 1 in front of it
      (1.5), the division by it 1, + eps 1 (the first three reach the denominator times sqrt(v) / sqrt(bc2) / denom <= 1);
      1 - b1^t 1, lr / bc1 1; m / denom 1; lr1 * (.) 1: 8.5, taken as C_D = 9.
      Propagated: lr1 err_m / denom; the sqrt(v) share of err_v, |d| (sqrt(v) / sqrt(bc2) / denom) err_v / (2 v); and powf's error,
      K_POW ulps of b^t, which the cancellation in 1 - b^t magnifies: |d| (K_POW ulp(b1^t) / bc1 + K_POW ulp(b2^t) / (2 bc2)).
      All of this is first order; adam_ref asserts that the relative terms add up to less than 2^-13, and the sum is multiplied
      by 1 + 2^-12 for the products of two of them.
  p   the final subtraction, u |p|, plus the bound of d.

K_POW = 1.  This is a SUPPOSITION: HIP's published table of device math function accuracy gives powf a maximum error of 1 ulp as
far as remembered; no copy of that table ships with the ROCm installation this was written against, so the figure could not be
checked there.  It is not fitted to the kernel's output.

adam_table(seed) is the input of the GPU test: per element of the padded bucket [2][107 024] (gpu_support.unpack_flat's layout) a
gradient class (|g| in G_MAGS times 1 .. 1.25, either sign) and a state class (STATES), dealt out per region by a seeded shuffle of
the 64 (magnitude, sign, state) combinations, so that every region with at least 64 live elements holds every combination and the
four elements of a quad differ.  b3 has 13 live elements in all: it walks the 64 combinations from offset 13 * seed, so that seeds
0 .. 4 — the GPU test uses all five — cover them together.  Padding (W1 columns 137 .. 143, W3 rows and b3 entries >= n3) carries
non-zero g, m0 and v0: the kernel must leave its m and v alone.

pack_ref restates pnr_mlp_pack: the fragment-native positions (frag32_off, frag16_off) of the five regions W1 | W2 | W3 | W2T | W3T
of csrc/pnr_mlp.h, padding zero, the planes by mlp_grad_ref.split_planes."""
import numpy as np
import torch

import mlp_grad_ref as gref

U = 2.0 ** -24
C_M, C_V, C_D = 3, 3, 9
K_POW = 1.0                                   # powf's error in ulps: a supposition, see the module docstring

IN, IN_PAD, HID, HEAD = 137, 144, 256, 16
N3 = (12, 1)
# the bucket's offsets: W1 [256][144] | W2 [256][256] | W3 [16][256] | b1 | b2 | b3 [16]
G_W2, G_W3, G_B1 = HID * IN_PAD, HID * IN_PAD + HID * HID, HID * IN_PAD + HID * HID + HEAD * HID
G_B2, G_B3 = G_B1 + HID, G_B1 + 2 * HID
E = G_B3 + HEAD                               # 107 024
REGIONS = ("W1", "W2", "W3", "b1", "b2", "b3", "padding")
PADDING = REGIONS.index("padding")
G_MAGS = (0.0, 1e-12, 1e-8, 3e-8, 1e-5, 1e-2, 1.0, 1e3)
STATES = ("fresh", "warm", "opposing", "stale")
N_COMBOS = len(G_MAGS) * 2 * len(STATES)      # 64: magnitude x sign x state
TABLE_SEEDS = (0, 1, 2, 3, 4)                 # together they give b3 every combination


def gamma(n):
    return n * U / (1.0 - n * U)


def f32(x):
    """the float32 value nearest x, widened to float64"""
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def ulp32(x):
    """the spacing of float32 at |x| (the subnormal spacing below the normal range)"""
    x = np.abs(np.asarray(x, np.float64))
    e = np.floor(np.log2(np.maximum(x, 2.0 ** -126)))
    return np.exp2(np.maximum(e, -126.0) - 23.0)


def adam_ref(p0, m0, v0, g, scale, t, lr, betas, eps):
    """One update in float64.  Returns {"p", "m", "v", "d", "g" (the scaled gradient g'), "lr1" (lr / (1 - b1^t)), "denom",
    "bound_p", "bound_m", "bound_v", "bound_d"}."""
    p0, m0, v0, g = (np.asarray(x, np.float64) for x in (p0, m0, v0, g))
    lr, b1, b2, eps, scale = (float(np.float32(x)) for x in (lr, betas[0], betas[1], eps, scale))
    assert 0.5 <= b1 <= 1.0 and 0.5 <= b2 <= 1.0, "1 - beta is exact in float32 only for betas in [0.5, 1]"
    t = int(t)
    assert t >= 1
    gs = f32(g * scale)
    ob1, ob2 = 1.0 - b1, 1.0 - b2
    m = m0 + (gs - m0) * ob1
    v = b2 * v0 + ob2 * gs * gs
    assert not np.any((v != 0) & (v < 2.0 ** -100)), "the table must stay clear of float32's subnormals"
    pw1, pw2 = b1 ** t, b2 ** t
    bc1, bc2 = 1.0 - pw1, 1.0 - pw2
    root = np.sqrt(v) / np.sqrt(bc2)
    denom = root + eps
    lr1 = lr / bc1
    d = lr1 * m / denom
    p = p0 - d

    bound_m = gamma(C_M) * (np.abs(m0) + ob1 * (np.abs(gs) + np.abs(m0)))
    bound_v = gamma(C_V) * v
    rel_pow = K_POW * float(ulp32(pw1)) / bc1 + K_POW * float(ulp32(pw2)) / (2.0 * bc2)
    rel_v = np.where(v > 0, (root / denom) * gamma(C_V) / 2.0, 0.0)          # (root / denom) err_v / (2 v)
    assert gamma(C_D) + rel_pow + float(rel_v.max(initial=0.0)) < 2.0 ** -13
    bound_d = (np.abs(d) * (gamma(C_D) + rel_pow + rel_v) + lr1 * bound_m / denom) * (1.0 + 2.0 ** -12)
    bound_p = U * np.abs(p) + bound_d
    return {"p": p, "m": m, "v": v, "d": d, "g": gs, "lr1": np.float64(lr1), "denom": denom, "bound_p": bound_p, "bound_m": bound_m, "bound_v": bound_v, "bound_d": bound_d}


# ---- the table ----------------------------------------------------------------------------------------------------------------------
def regions():
    """the region label (an index into REGIONS) of every element of the padded bucket, [2, E] int8"""
    out = np.full((2, E), PADDING, np.int8)
    for n in range(2):
        w1 = out[n, :G_W2].reshape(HID, IN_PAD)
        w1[:, :IN] = 0
        out[n, G_W2:G_W3] = 1
        out[n, G_W3:G_W3 + N3[n] * HID] = 2
        out[n, G_B1:G_B2] = 3
        out[n, G_B2:G_B3] = 4
        out[n, G_B3:G_B3 + N3[n]] = 5
    return out


def adam_table(seed):
    """{"g", "m0", "v0": float32 [2, E]; "region", "mag", "sign", "state": int8 [2, E] (indices into REGIONS, G_MAGS, (+, -), STATES)}"""
    rng = np.random.RandomState(7000 + seed)
    region = regions()
    combo = np.zeros((2, E), np.int64)
    b3_at = 13 * seed
    for n in range(2):
        for r in range(len(REGIONS)):
            at = np.flatnonzero(region[n] == r)
            if r == 5:                                   # b3: too few elements for a shuffle to cover anything
                c = (b3_at + np.arange(at.size)) % N_COMBOS
                b3_at += at.size
            else:
                c = rng.permutation(np.arange(at.size) % N_COMBOS)
            combo[n, at] = c
    mag, sign, state = combo % 8, (combo // 8) % 2, combo // 16
    pad = region == PADDING                              # padding: non-zero g, m0, v0
    mag = np.where(pad & (mag == 0), 1 + combo // 16 % 7, mag)
    state = np.where(pad & (state == 0), 1 + combo % 3, state)
    jitter = lambda: 1.0 + 0.25 * rng.uniform(size=(2, E))      # noqa: E731
    g = f32(np.where(sign == 0, 1.0, -1.0) * np.asarray(G_MAGS)[mag] * jitter())
    about = lambda: rng.uniform(0.5, 1.5, size=(2, E))          # noqa: E731
    m_warm, v_warm = g * about(), g * g * about()
    m0 = np.select([state == 0, state == 1, state == 2], [0.0, m_warm, -g], m_warm)
    v0 = np.select([state == 0, state == 1, state == 2], [0.0, v_warm, v_warm], 1e4 * g * g)
    i8 = lambda a: a.astype(np.int8)                            # noqa: E731
    return {"g": g.astype(np.float32), "m0": m0.astype(np.float32), "v0": v0.astype(np.float32),
            "region": region, "mag": i8(mag), "sign": i8(sign), "state": i8(state)}


# ---- the packed weights -------------------------------------------------------------------------------------------------------------
OFF_W1 = 0
OFF_W2 = OFF_W1 + HID * IN_PAD
OFF_W3 = OFF_W2 + HID * HID
OFF_W2T = OFF_W3 + HEAD * HID
OFF_W3T = OFF_W2T + HID * HID
PACK_ELEMS = OFF_W3T + HID * HEAD              # 176 128
BIAS_ELEMS = 2 * HID + HEAD


def frag32_off(row, k, ks):
    """element offset of A[row][k] in a matrix packed as 32 x 16 blocks, K = 16 ks (csrc/pnr_mlp.h)"""
    return ((((row >> 5) * ks + (k >> 4)) * 64) + (row & 31) + 32 * ((k >> 3) & 1)) * 8 + (k & 7)


def frag16_off(row, k):
    """the same for a 16-row matrix packed as blocks of 16 x 32"""
    return (((k >> 5) * 64) + row + 16 * ((k >> 3) & 3)) * 8 + (k & 7)


def pack_index():
    """{region: the destination index of every element of the region's source matrix, in its row-major shape} for W1 [256, 144],
    W2 [256, 256], W3 [16, 256], W2T [256, 256] (W2T[i][o] = W2[o][i]) and W3T [256, 16] (W3T[f][r] = W3[r][f])"""
    grid = lambda r, c: np.meshgrid(np.arange(r), np.arange(c), indexing="ij")      # noqa: E731
    o, k = grid(HID, IN_PAD)
    out = {"W1": OFF_W1 + frag32_off(o, k, IN_PAD // 16)}
    o, i = grid(HID, HID)
    out["W2"] = OFF_W2 + frag32_off(o, i, HID // 16)
    r, f = grid(HEAD, HID)
    out["W3"] = OFF_W3 + frag16_off(r, f)
    i, o = grid(HID, HID)
    out["W2T"] = OFF_W2T + frag32_off(i, o, HID // 16)
    f, r = grid(HID, HEAD)
    out["W3T"] = OFF_W3T + frag32_off(f, r, 1)
    return out


def pack_ref(params, n3, planes):
    """(wpack [planes, 2, 176 128] with bf16 element type, bias [2, 528] float32) of the twelve float32 master parameters (policy
    W1, b1, W2, b2, W3, b3, then the value net's; torch tensors or arrays) with head widths n3"""
    idx = pack_index()
    src = np.zeros((2, PACK_ELEMS), np.float32)
    bias = np.zeros((2, BIAS_ELEMS), np.float32)
    for n in range(2):
        w1, b1, w2, b2, w3, b3 = (np.asarray(torch.as_tensor(t).detach().cpu(), np.float32) for t in params[6 * n:6 * n + 6])
        assert w1.shape == (HID, IN) and w2.shape == (HID, HID) and w3.shape == (n3[n], HID) and b3.shape == (n3[n],)
        w1p = np.zeros((HID, IN_PAD), np.float32); w1p[:, :IN] = w1
        w3p = np.zeros((HEAD, HID), np.float32); w3p[:n3[n]] = w3
        for name, mat in (("W1", w1p), ("W2", w2), ("W3", w3p), ("W2T", w2.T), ("W3T", w3p.T)):
            src[n, idx[name].ravel()] = mat.ravel()
        bias[n, :HID], bias[n, HID:2 * HID], bias[n, 2 * HID:2 * HID + n3[n]] = b1, b2, b3
    return gref.split_planes(torch.from_numpy(src), planes, "weight", 0), torch.from_numpy(bias)
