"""float64 restatement of the three MCMC kernels (include/brush_hip.h: brush_mcmc_inject_noise, brush_mcmc_reg_grads,
brush_mcmc_relocation) and a pure-Python Philox4x32-10.

Noise:        xi from Philox (key (seed & 0xffffffff, seed >> 32), counter (g, step, 0x4D434D43, 0)), uniforms
              u_i = ((x_i >> 8) + 0.5) 2^-24, Box-Muller; delta = R diag(exp(2 s)) R^T (xi gate scale).
Regulariser:  d/d raw of reg_o mean sigmoid(raw) and d/d s of reg_s mean exp(s).
Relocation:   Eq. 9 of Kheradmand et al. 2024, the double sum as the paper writes it.

`noise_delta64` also returns, per component, the sum of the absolute values of the terms the component is made of (the
rotation entries included: |1| + 2 (y^2 + z^2), 2 (|x y| + |w z|), ...): the scale rounding errors are measured against.
"""
import math

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
COUNTER_TAG = 0x4D434D43
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Random123's Philox4x32 with 10 rounds on Python ints: counter (c0..c3), key (k0, k1) -> (x0..x3)."""
    c0, c1, c2, c3 = (int(c) & MASK for c in counter)
    k0, k1 = (int(k) & MASK for k in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def philox_words(seed, step, n):
    """[n,4] uint64 array of the output words of splats 0..n-1 (the same rounds on numpy columns)."""
    c = [np.arange(n, dtype=np.uint64), np.full(n, int(step) & MASK, np.uint64),
         np.full(n, COUNTER_TAG, np.uint64), np.zeros(n, np.uint64)]
    k0, k1 = int(seed) & MASK, (int(seed) >> 32) & MASK
    m = np.uint64(MASK)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]   # 32 x 32 bits: fits 64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(c, 1)


def uniforms(words):
    """u = ((x >> 8) + 0.5) 2^-24 in float64 (exact), strictly inside (0, 1)."""
    return ((np.asarray(words, np.uint64) >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def xi64(seed, step, n):
    """[n,3] float64 standard normals of (seed, step, g)."""
    u = uniforms(philox_words(seed, step, n))
    r01, r2 = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    a1, a3 = 2.0 * math.pi * u[:, 1], 2.0 * math.pi * u[:, 3]
    return np.stack([r01 * np.cos(a1), r01 * np.sin(a1), r2 * np.cos(a3)], 1)


def sigmoid(x):
    x = np.asarray(x, np.float64)
    return np.where(x >= 0, 1.0 / (1.0 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x))))


def gate64(raw):
    """gsplat's op_sigmoid(1 - o): 1 / (1 + exp(-100 ((1 - sigmoid(raw)) - 0.995)))."""
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-100.0 * (sigmoid(-np.asarray(raw, np.float64)) - 0.995)))


def rotmat64(rotation):
    """(R [n,3,3], sum of absolute terms of every entry [n,3,3]) of rotation / |rotation|, (w, x, y, z)."""
    q = np.asarray(rotation, np.float64)
    q = q / np.sqrt((q * q).sum(1, keepdims=True))
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((q.shape[0], 3, 3))
    A = np.empty_like(R)
    R[:, 0, 0], A[:, 0, 0] = 1 - 2 * (y * y + z * z), 1 + 2 * (y * y + z * z)
    R[:, 1, 1], A[:, 1, 1] = 1 - 2 * (x * x + z * z), 1 + 2 * (x * x + z * z)
    R[:, 2, 2], A[:, 2, 2] = 1 - 2 * (x * x + y * y), 1 + 2 * (x * x + y * y)
    for (i, j, a, b, sgn) in ((1, 0, x * y, w * z, 1), (0, 1, x * y, w * z, -1), (2, 0, x * z, w * y, -1),
                              (0, 2, x * z, w * y, 1), (2, 1, y * z, w * x, 1), (1, 2, y * z, w * x, -1)):
        R[:, i, j], A[:, i, j] = 2 * (a + sgn * b), 2 * (np.abs(a) + np.abs(b))
    return R, A


def noise_delta64(log_scales, rotation, raw_opacity, xi, scale):
    """(delta [n,3], sum of absolute terms [n,3]) of Sigma (xi gate scale), from the f32 inputs in float64."""
    R, A = rotmat64(rotation)
    e = np.exp(2.0 * np.asarray(log_scales, np.float64))
    w = np.asarray(xi, np.float64) * (gate64(raw_opacity) * float(scale))[:, None]
    t = np.einsum("nik,ni->nk", R, w) * e
    ta = np.einsum("nik,ni->nk", A, np.abs(w)) * e
    return np.einsum("nik,nk->ni", R, t), np.einsum("nik,nk->ni", A, ta)


def reg_terms64(raw_opacity, log_scales, opacity_reg, scale_reg):
    """(term added to v_opac [n], term added to v_scales [n,3])."""
    raw, ls = np.asarray(raw_opacity, np.float64), np.asarray(log_scales, np.float64)
    n = raw.shape[0]
    s = sigmoid(raw)
    return float(opacity_reg) / n * s * (1.0 - s), float(scale_reg) / (3.0 * n) * np.exp(ls)


def relocation64(o, ratio):
    """Eq. 9 from the opacity: (o' unclamped, coefficient o / D that multiplies the scales, sum |terms| of D)."""
    N = min(max(int(ratio), 1), 51)
    o = float(o)
    o_new = -math.expm1(math.log1p(-o) / N)   # 1 - (1 - o)^(1/N) without the cancellation
    D, Dabs = 0.0, 0.0
    for i in range(1, N + 1):
        for k in range(i):
            term = math.comb(i - 1, k) * (-1.0) ** k * o_new ** (k + 1) / math.sqrt(k + 1)
            D += term
            Dabs += abs(term)
    return o_new, o / D, Dabs


def softplus(x):
    return x + math.log1p(math.exp(-x)) if x > 0 else math.log1p(math.exp(x))


def relocation_rows64(raw_opacity, log_scales, ratio, min_opacity):
    """The kernel's outputs in float64 from its f32 inputs: (new raw opacity [m], new log-scales [m,3])."""
    raw, ls = np.asarray(raw_opacity, np.float64), np.asarray(log_scales, np.float64)
    new_raw, new_ls = np.empty_like(raw), np.empty_like(ls)
    hi = 1.0 - 2.0 ** -24
    for g in range(raw.shape[0]):
        N = min(max(int(ratio[g]), 1), 51)
        o = 1.0 / (1.0 + math.exp(-raw[g]))
        L = -softplus(raw[g]) / N                     # ln(1 - o')
        o_new = -math.expm1(L)
        D = 0.0
        for i in range(1, N + 1):
            for k in range(i):
                D += math.comb(i - 1, k) * (-1.0) ** k * o_new ** (k + 1) / math.sqrt(k + 1)
        new_ls[g] = ls[g] + math.log(o / D)
        if o_new < min_opacity:
            new_raw[g] = math.log(min_opacity / (1.0 - min_opacity))
        elif o_new > hi:
            new_raw[g] = math.log(hi / 2.0 ** -24)
        else:
            new_raw[g] = math.log(o_new) - L
    return new_raw, new_ls


def sample_by_weight_np(weights, u):
    """numpy restatement of brush_amd.mcmc.sample_by_weight."""
    cdf = np.cumsum(np.asarray(weights, np.float64))
    total = cdf[-1]
    target = np.minimum(np.asarray(u, np.float64) * total, np.nextafter(total, 0.0))
    return np.minimum(np.searchsorted(cdf, target, side="right"), len(cdf) - 1)
