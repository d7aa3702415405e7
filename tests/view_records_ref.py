"""Directed inputs and plain numpy references of the view-record reduction (brush_amd/csrc/view_records.hip:
brush_reduce_view_records, brush_reduce_view_records_adam).  No GPU, no torch.

directed_views builds hand-made 64-byte records `[gid | v_means(3) | v_scales(3) | v_quats(4) | v_opac | v_rgb(3) |
norm]` of W views over n splats in both buffer layouts, with everything around the valid records that the kernels'
own checks must reject.  reduce_f32 is the strictly sequential float32 sum in view order (the bits the kernels must
produce for everything but v_sh), reduce_f64 the float64 sum with v_sh, sh_f32 a float32 restatement of v_sh that
only sizes the v_sh tolerance and serves as the subject of the negative controls.

Order-sensitive payloads.  Of the splats that three or more views see, a quarter carry (+B, s, -B) in three of their
views in view order, in one word of each of means, scales, quats, opac and rgb, with B = s 2^k, k >= 30.  By
enumeration that triple sums to 0 in four of the six orders of its terms (every order in which s meets a big term
before the two big terms cancel), the reversed view order among them: it tells a reduction that brings the two big
terms together from the sequential one, but not a reversed one.  So twice as many splats carry the rotated triple
(+B, -B, s): it sums to s in view order and to 0 as soon as s is not added last.  The statistic norm is >= 0 by
contract and takes (s, s, 2^24 s) with s a power of two instead: 2^24 s + 2 s is exact in view order, while 2^24 s + s
is a tie that rounds back to 2^24 s, so the norm of every planted splat changes under a reversal.  The other views'
values in a planted word are +-0, so the planted sums are known.  tests/test_view_records_cpu.py measures the share
of planted splats whose bits change under other orders of the views."""
import numpy as np

REC = 16                                      # floats per record
EPS32 = float(np.finfo(np.float32).eps)       # 2^-23
INVALID = 0xFFFFFFFF
GROUPS = (("v_means", 0, 3), ("v_scales", 3, 6), ("v_quats", 6, 10), ("v_opac", 10, 11), ("v_rgb", 11, 14),
          ("xy_norm", 14, 15))                # payload columns (record word - 1)

WS = (1, 2, 7, 8, 9, 15, 16, 17)
NS = (1, 63, 64, 65, 255, 257, 1000, 4096, 4099)
DEGS = (0, 1, 2, 3, 4)
# (W, n, deg) of the dense GPU cases: every W at n = 4099, deg 3 (kChunk = 8: one pass, the edge, two passes, the edge of
# two, three); every deg and every n at W = 9 (tails, single waves, the float4 and scalar v_sh rows).
DENSE_CASES = [(W, 4099, 3) for W in WS] + [(9, n, deg) for deg in DEGS for n in NS if (n, deg) != (4099, 3)]

# max |sh_f32 - reduce_f64| / (EPS32 mag_sh) over DENSE_CASES per degree, measured by
# tests/test_view_records_cpu.py::test_sh_tolerance_base_values (numpy float32 against numpy float64, no GPU involved),
# rounded up (measured: 0.515, 0.842, 1.834, 4.095, 7.146 for degree 0..4); the GPU gate allows 4 x as much (the
# device's expression tree for the basis differs from the restatement's, and each of up to 17 additions rounds once).
K_BASE = {0: 0.52, 1: 0.85, 2: 1.84, 3: 4.1, 4: 7.15}
K_MARGIN = 4.0


def k_sh(deg):
    return K_MARGIN * K_BASE[deg]


def case_seed(W, n, deg):
    return 100000 * deg + 1000 * W + n


def empty_views(W):
    """Views that contribute no rows, in the middle of the batch (never view 0, 7, 8 or W-1)."""
    return np.array((2, 4) if W >= 6 else (2,) if W >= 4 else (), dtype=np.int64)


def _signed_log(rng, shape, lo, hi):
    return (rng.choice([-1.0, 1.0], size=shape) * 10.0 ** rng.uniform(lo, hi, size=shape)).astype(np.float32)


def _payload(rng, shape):
    """Signed log-uniform 1e-20 .. 1e6 (all normal float32), 3 % +0, 3 % -0; the last column (norm) >= 0."""
    p = _signed_log(rng, shape, -20, 6)
    c = rng.random(shape)
    p[c < 0.03] = 0.0
    p[(c >= 0.03) & (c < 0.06)] = -0.0
    p[..., 14] = np.abs(p[..., 14])
    return p


def _geometry(rng, n, W):
    campos = rng.uniform(-2.0, 2.0, (W, 3)).astype(np.float32)
    means = rng.uniform(-2.0, 2.0, (n, 3)).astype(np.float32)
    for _ in range(100):
        d = np.linalg.norm(means.astype(np.float64)[:, None, :] - campos.astype(np.float64)[None], axis=2)
        near = (d < 0.1).any(axis=1)
        if not near.any():
            return means, campos
        means[near] = rng.uniform(-2.0, 2.0, (int(near.sum()), 3)).astype(np.float32)
    raise AssertionError("no placement keeps every splat 0.1 away from every camera")


def _visibility(rng, n, W, seed):
    live = [v for v in range(W) if v not in empty_views(W)]
    cls = rng.integers(0, 9, n)
    vis = np.zeros((n, W), bool)
    vis[cls == 1] = True
    for c, v in ((2, 0), (3, W - 1), (4, min(7, W - 1)), (5, min(8, W - 1))):
        vis[cls == c, v] = True
    for c, p in ((6, 0.02), (7, 0.5), (8, 0.98)):
        m = cls == c
        vis[m] = rng.random((int(m.sum()), W)) < p
    # whole 64-aligned waves: unseen, seen, lane 0 only, lane 63 only, alternating lanes
    nw = n // 64
    lanes = np.arange(64)
    patterns = (lanes < 0, lanes >= 0, lanes == 0, lanes == 63, lanes % 2 == 0)
    waves = {}
    for i in range(min(5, nw - 1)):   # never wave 0: a cloud of one or two waves keeps its mix of classes
        wi = 1 + 2 * i if nw >= 10 else 1 + i
        k = (i + seed) % 5
        waves[wi] = k
        rows = vis[wi * 64:(wi + 1) * 64]
        rows[:] = rng.random((64, W)) < 0.5
        rows[:, empty_views(W)] = False
        none = ~rows[:, live].any(axis=1)
        rows[none, rng.choice(live, size=int(none.sum()))] = True
        rows[~patterns[k]] = False
    vis[:, empty_views(W)] = False
    return vis, waves


def _plant_order_sensitive(rng, vis, P):
    """See the module docstring.  Returns {gid: dict(kind, views, cols, small)}: kind 'sym' (+B, s, -B) or 'rot'
    (+B, -B, s), the three views, and per group the planted payload column and its small value s."""
    n, W = vis.shape
    eligible = rng.permutation(np.flatnonzero(vis.sum(axis=1) >= 3))
    n_sym = -(-len(eligible) // 4)
    n_rot = min(len(eligible) - n_sym, 2 * n_sym)
    planted = {}
    for i, g in enumerate(eligible[:n_sym + n_rot]):
        kind = "sym" if i < n_sym else "rot"
        seen = np.flatnonzero(vis[g])
        a, b, c = np.sort(rng.choice(seen, 3, replace=False))
        info = dict(kind=kind, views=(int(a), int(b), int(c)), cols={}, small={})
        for name, lo, hi in GROUPS:
            col = int(rng.integers(lo, hi))
            zeros = np.where(rng.random(len(seen)) < 0.5, 0.0, -0.0).astype(np.float32)
            info["cols"][name] = col
            if name == "xy_norm":
                s = np.float32(2.0 ** int(rng.integers(-30, -10)))
                P[seen, g, col] = 0.0
                P[[a, b, c], g, col] = (s, s, np.ldexp(s, 24))
                info["small"][name] = s
                continue
            s = _signed_log(rng, (), -12, -6)
            big = np.ldexp(s, int(rng.integers(30, 40)))        # exact: <= 1e-6 2^39 < 1e6
            P[seen, g, col] = zeros
            P[[a, b, c], g, col] = (big, s, -big) if kind == "sym" else (big, -big, s)
            info["small"][name] = s
        planted[int(g)] = info
    return planted


def _hostile_rows(n):
    r = np.full((3, REC), np.nan, np.float32)
    r.view(np.uint32)[:, 0] = (n, 0x80000000, 0xFFFFFFFF)
    return r


def _shuffled(rng, k):
    p = rng.permutation(k)
    if k >= 2 and np.all(np.diff(p) > 0):
        p = p[::-1].copy()
    return p


def directed_views(n, W, deg, seed, layout):
    """The records of W views over n splats in one buffer layout ('padded': view_offsets None, view v at row
    v * rows_per_view; 'packed': view v at row view_offsets[v] of rows_per_view rows in all).  Both layouts of one
    (n, W, seed) hold the same valid records; `deg` is only carried along.  Returns a dict: means [n,3], campos [W,3],
    records [rows,16] float32 (word 0 holds the gid's bits), view_rows [W] u32, view_offsets [W] u32 or None,
    rows_per_view, vis [n,W] (which view contributes a record of which splat), planted {gid: info}, waves
    {wave: pattern} and P [W,n,15], the payload of (view, splat) where vis."""
    assert layout in ("padded", "packed") and n >= 1 and W >= 1
    rng = np.random.default_rng([seed, n, W])
    means, campos = _geometry(rng, n, W)
    vis, waves = _visibility(rng, n, W, seed)
    P = _payload(rng, (W, n, 15))
    planted = _plant_order_sensitive(rng, vis, P)
    empty = empty_views(W)
    views = []   # the physical rows of every view: its valid records and three out-of-range gids, in shuffled order
    for v in range(W):
        if v in set(empty.tolist()):
            views.append(np.zeros((0, REC), np.float32))
            continue
        gids = np.flatnonzero(vis[:, v])
        rows = np.empty((len(gids), REC), np.float32)
        rows.view(np.uint32)[:, 0] = gids
        rows[:, 1:] = P[v, gids]
        rows = np.concatenate([rows, _hostile_rows(n)])
        views.append(rows[_shuffled(rng, len(rows))])
    counts = np.array([len(r) for r in views], np.uint32)

    def stale(k):   # rows nobody may read: valid gids of seen and unseen splats, NaN payload
        r = np.full((k, REC), np.nan, np.float32)
        r.view(np.uint32)[:, 0] = rng.integers(0, n, k)
        return r

    view_rows = counts.copy()
    if layout == "padded":
        rpv = int(counts.max())
        records = np.concatenate([np.concatenate([r, stale(rpv - len(r))]) for r in views])
        view_rows[int(np.argmax(counts))] += 3           # claims more rows than the stride holds: clamped to it
        offsets = None
    else:
        rpv = int(counts.sum())
        records = np.concatenate(views)
        offsets = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint32)
        view_rows[W - 1] += 5                             # the last view runs past the buffer: clamped to what is left
        if len(empty):                                    # a view whose offset is >= the total has no room at all
            offsets[empty[-1]] = rpv + (7 if seed % 2 else 0)
            view_rows[empty[-1]] = 9
    return dict(n=n, W=W, deg=deg, seed=seed, layout=layout, means=means, campos=campos,
                records=np.ascontiguousarray(records), view_rows=view_rows, view_offsets=offsets, rows_per_view=rpv,
                vis=vis, planted=planted, waves=waves, P=P)


def view_slices(case):
    """Per view the (gids, payload [k,15]) of the rows the reduction may use, as the comments of k_build_view_index and
    sum_view_records state it: rows [first, first + min(view_rows[v], room)) whose gid is < n."""
    rec, n, rpv = case["records"], case["n"], case["rows_per_view"]
    out = []
    for v in range(case["W"]):
        if case["view_offsets"] is None:
            first, room = v * rpv, rpv
        else:
            first = int(case["view_offsets"][v])
            room = rpv - first if first < rpv else 0
        rows = rec[first:first + min(int(case["view_rows"][v]), room)]
        gid = rows[:, 0].view(np.uint32)
        keep = gid < n
        g = gid[keep].astype(np.int64)
        assert len(np.unique(g)) == len(g), "a gid appears at most once per view"
        out.append((g, rows[keep, 1:]))
    return out


def _zeros(n, dtype):
    return {"v_means": np.zeros((n, 3), dtype), "v_scales": np.zeros((n, 3), dtype), "v_quats": np.zeros((n, 4), dtype),
            "v_opac": np.zeros((n,), dtype), "xy_norm": np.zeros((n,), dtype), "views_seen": np.zeros((n,), dtype)}


def _add_view(out, g, p, one):
    # a gid appears once per view: every element takes exactly one addition of the arrays' dtype
    out["v_means"][g] = out["v_means"][g] + p[:, 0:3]
    out["v_scales"][g] = out["v_scales"][g] + p[:, 3:6]
    out["v_quats"][g] = out["v_quats"][g] + p[:, 6:10]
    out["v_opac"][g] = out["v_opac"][g] + p[:, 10]
    out["xy_norm"][g] = out["xy_norm"][g] + p[:, 14]
    out["views_seen"][g] = out["views_seen"][g] + one


def reduce_f32(case, order=None):
    """float32, strictly sequential from 0.f in view order 0..W-1 (`order`: another order of the views, for the proof
    that the planted payloads are order-sensitive)."""
    out = _zeros(case["n"], np.float32)
    slices = view_slices(case)
    for v in (range(case["W"]) if order is None else order):
        g, p = slices[v]
        assert p.dtype == np.float32
        _add_view(out, g, p, np.float32(1.0))
    assert all(a.dtype == np.float32 for a in out.values())
    return out


def reduce_f32_pairwise(case):
    """The same terms added as a balanced tree over the views (absent records enter as +0)."""
    slices = view_slices(case)
    leaves = []
    for g, p in slices:
        o = _zeros(case["n"], np.float32)
        _add_view(o, g, p, np.float32(1.0))
        leaves.append(o)
    while len(leaves) > 1:
        nxt = [{k: a[k] + b[k] for k in a} for a, b in zip(leaves[0::2], leaves[1::2])]
        if len(leaves) % 2:
            nxt.append(leaves[-1])
        leaves = nxt
    return leaves[0]


_SH_C = (0.2820947917738781, 0.48860251190292, 1.092548430592079, 0.5462742152960395, 0.9461746957575601,
         0.3153915652525201, 2.285228997322329, 0.4570457994644658, 1.445305721320277, 0.5900435899266435,
         1.865881662950577, 1.119528997770346, 4.683325804901025, 2.007139630671868, 3.31161143515146,
         0.47308734787878, 1.770130769779931, 0.6258357354491763, 1.984313483298443, 1.006230589874905)


def sloan_basis(deg, d):
    """The real SH basis of Sloan, 'Efficient Spherical Harmonic Evaluation' (JCGT 2013), bands 0..deg, in the dtype of
    the unit directions d [M,3] -> [M,(deg+1)^2]."""
    t = d.dtype.type
    c = [t(v) for v in _SH_C]
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    Y = [np.full_like(x, c[0])]
    if deg >= 1:
        Y += [-c[1] * y, c[1] * z, -c[1] * x]
    if deg >= 2:
        z2 = z * z
        f0b = -c[2] * z
        c1 = x * x - y * y
        s1 = t(2.0) * x * y
        p6 = c[4] * z2 - c[5]
        Y += [c[3] * s1, f0b * y, p6, f0b * x, c[3] * c1]
    if deg >= 3:
        f0c = -c[6] * z2 + c[7]
        f1b = c[8] * z
        c2 = x * c1 - y * s1
        s2 = x * s1 + y * c1
        p12 = z * (c[10] * z2 - c[11])
        Y += [-c[9] * s2, f1b * s1, f0c * y, p12, f0c * x, f1b * c1, -c[9] * c2]
    if deg >= 4:
        f0d = z * (-c[12] * z2 + c[13])
        f1c = c[14] * z2 - c[15]
        f2b = -c[16] * z
        c3 = x * c2 - y * s2
        s3 = x * s2 + y * c2
        Y += [c[17] * s3, f2b * s2, f1c * s1, f0d * y, c[18] * z * p12 - c[19] * p6, f0d * x, f1c * c1, f2b * c2,
              c[17] * c3]
    Y = np.stack(Y, axis=1)
    assert Y.dtype == d.dtype
    return Y


MUTATIONS = ("drop_view8", "swap_campos", "flip_band", "rotate_rgb", "no_normalise")


def _sh_sum(case, dtype, mutate=None):
    """v_sh[g] = sum over views, in view order, of Y(dir_v(g)) (x) v_rgb_v(g), dir = (mean - campos[v]) / |.|, all in
    `dtype` from the float32 inputs; mag[g,k,c] = sum_v |v_rgb_c(v)| in float64."""
    assert mutate is None or mutate in MUTATIONS
    n, W, deg = case["n"], case["W"], case["deg"]
    ncoef = (deg + 1) ** 2
    means, campos = case["means"].astype(dtype), case["campos"].astype(dtype)
    if mutate == "swap_campos":
        campos = campos.copy()
        campos[[7, 8]] = campos[[8, 7]]
    sh = np.zeros((n, ncoef, 3), dtype)
    mag = np.zeros((n, 1, 3), np.float64)
    for v, (g, p) in enumerate(view_slices(case)):
        rgb = p[:, 11:14].astype(dtype)
        mag[g, 0] = mag[g, 0] + np.abs(rgb.astype(np.float64))
        if mutate == "drop_view8" and v == 8:
            continue
        if mutate == "rotate_rgb":
            rgb = np.roll(rgb, 1, axis=1)
        d = means[g] - campos[v][None, :]
        if mutate != "no_normalise":
            d = d / np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])[:, None]
        Y = sloan_basis(deg, d)
        if mutate == "flip_band":
            Y[:, 1:4] = -Y[:, 1:4]
        sh[g] = sh[g] + Y[:, :, None] * rgb[:, None, :]
    assert sh.dtype == dtype
    return sh, np.broadcast_to(mag, sh.shape)


def reduce_f64(case):
    """Everything in float64: the six sums of reduce_f32, v_sh, and mag_sh[g,k,c] = sum_v |v_rgb_c(v)|."""
    out = _zeros(case["n"], np.float64)
    for g, p in view_slices(case):
        _add_view(out, g, p.astype(np.float64), 1.0)
    out["v_sh"], out["mag_sh"] = _sh_sum(case, np.float64)
    return out


def sh_f32(case, mutate=None):
    """Plain float32 restatement of v_sh.  Sizes the tolerance and is the subject of the negative controls; never a
    reference for the GPU."""
    return _sh_sum(case, np.float32, mutate)[0]


def sh_ratio(got, want64, mag):
    """|got - want| / (EPS32 mag) per element; where mag is 0 every term is +-0 and the sum must be 0."""
    err = np.abs(np.asarray(got, np.float64) - want64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = err / (EPS32 * mag)
    r = np.where(mag == 0.0, np.where(err == 0.0, 0.0, np.inf), r)
    return np.where(np.isfinite(r), r, np.inf)


def sh_gate(got, want64, mag, deg):
    """The v_sh gate of the GPU test: (worst |got - f64| / (EPS32 mag_sh), elements over k_sh(deg))."""
    r = sh_ratio(got, want64, mag)
    return float(r.max()) if r.size else 0.0, int((r > k_sh(deg)).sum())


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
