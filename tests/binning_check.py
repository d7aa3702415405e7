"""The integer half of the forward parity check, and properties of the tile lists that need no oracle.

Both work on plain numpy views of a render's aux state (`aux_arrays` for a GPU RenderAux, `oracle_arrays` for the CPU
oracle's), so the GPU modules share one checker and tests/test_binning_cpu.py can show on the CPU that it has teeth.
"""
import numpy as np

from tests import binning_clouds as BC


def _np_u32(t):
    return t.detach().cpu().numpy().astype(np.int32).view(np.uint32)


def aux_arrays(aux, uniforms_num_visible=None):
    """Numpy view of a GPU RenderAux (host readbacks)."""
    return dict(num_visible=aux.read_num_visible(), uniforms_num_visible=uniforms_num_visible,
                num_intersections=aux.read_num_intersections(), overflow=int(aux.overflow.item()),
                global_from_compact_gid=_np_u32(aux.global_from_compact_gid),
                compact_from_global_gid=_np_u32(aux.compact_from_global_gid),
                projected_splats=aux.projected_splats.detach().cpu().numpy(),
                cum_tiles_hit=_np_u32(aux.cum_tiles_hit),
                compact_gid_from_isect=_np_u32(aux.compact_gid_from_isect),
                tile_bins=_np_u32(aux.tile_bins))


def oracle_arrays(oa):
    """The oracle's aux in the same form (copies: the teeth tests corrupt them).  The oracle keeps no inverse map; the
    one the op must produce follows from global_from_compact_gid."""
    V = int(oa["num_visible"][0])
    n = oa["global_from_compact_gid"].shape[0]
    inv = np.full(n, 0xFFFFFFFF, np.uint32)
    inv[oa["global_from_compact_gid"][:V]] = np.arange(V, dtype=np.uint32)
    return dict(num_visible=V, uniforms_num_visible=V, num_intersections=int(oa["num_intersections"][0]),
                overflow=int(oa["overflow"]), global_from_compact_gid=oa["global_from_compact_gid"].copy(),
                compact_from_global_gid=inv, projected_splats=oa["projected_splats"].copy(),
                cum_tiles_hit=oa["cum_tiles_hit"].copy(), compact_gid_from_isect=oa["compact_gid_from_isect"].copy(),
                tile_bins=oa["tile_bins"].copy())


def assert_integer_parity(got, oa, nan_equal=False):
    """Every integer / index output of the forward bit-exact against the oracle's aux `oa` (and the projected records
    bitwise).  Returns (V, I).
    nan_equal (tests/test_gpu_cull.py, extreme scales only): the records must hold NaN in the same words and be bitwise
    equal in every other word; the sign and payload of a NaN that `inf - inf` produces differ between the host and the
    device."""
    V, I = int(oa["num_visible"][0]), int(oa["num_intersections"][0])
    assert got["num_visible"] == V
    assert got["uniforms_num_visible"] == V  # uniforms_buffer word 25 (render.rs:145-149)
    assert got["num_intersections"] == I
    assert got["overflow"] == int(oa["overflow"])
    n = oa["global_from_compact_gid"].shape[0]
    # integer / index outputs: bit-exact
    assert np.array_equal(got["global_from_compact_gid"][:n], oa["global_from_compact_gid"])
    want_inv = np.full(n, 0xFFFFFFFF, np.uint32)
    want_inv[oa["global_from_compact_gid"][:V]] = np.arange(V, dtype=np.uint32)
    assert np.array_equal(got["compact_from_global_gid"][:n], want_inv)
    gp = np.ascontiguousarray(got["projected_splats"][:V])
    op = np.ascontiguousarray(oa["projected_splats"][:V])
    if nan_equal:
        g_nan, o_nan = np.isnan(gp), np.isnan(op)
        assert np.array_equal(g_nan, o_nan), "projected splats hold NaN in different words"
        assert np.array_equal(gp.view(np.uint32)[~o_nan], op.view(np.uint32)[~o_nan]), "projected splats differ bitwise"
    else:
        assert np.array_equal(gp.view(np.uint32), op.view(np.uint32)), "projected splats differ bitwise"
    assert np.array_equal(got["cum_tiles_hit"][:n], oa["cum_tiles_hit"])
    assert np.array_equal(got["compact_gid_from_isect"][:I], oa["compact_gid_from_isect"][:I])
    assert np.array_equal(got["tile_bins"], oa["tile_bins"])
    return V, I


def assert_binning_properties(got):
    """What must hold of tile_bins and compact_gid_from_isect whatever the scene, from the op's own outputs alone:
      * the bins are disjoint and cover [0, I) in ascending tile order;
      * inside a bin the compact gids are strictly ascending (depth order, one entry per splat);
      * the per-gid entry counts equal the differences of cum_tiles_hit when nothing overflowed (and never exceed
        them when the list was truncated);
      * every (tile, gid) pair lies inside the reference bbox recomputed from projected_splats."""
    V, I = int(got["num_visible"]), int(got["num_intersections"])
    bins = got["tile_bins"].astype(np.int64)
    tby, tbx = bins.shape[0], bins.shape[1]
    flat = bins.reshape(-1, 2)
    lens = flat[:, 1] - flat[:, 0]
    assert (lens >= 0).all(), "a bin ends before it starts"
    tiles = np.flatnonzero(lens > 0)
    if I == 0:
        assert tiles.size == 0
        return
    start, end = flat[tiles, 0], flat[tiles, 1]
    assert start[0] == 0 and end[-1] == I, (int(start[0]), int(end[-1]), I)
    assert np.array_equal(start[1:], end[:-1]), "bins overlap, leave a gap or are out of tile order"
    gids = got["compact_gid_from_isect"][:I].astype(np.int64)
    assert gids.max() < V, "an entry names a splat that is not visible"
    tile_of = np.repeat(tiles, lens[tiles])
    same = tile_of[1:] == tile_of[:-1]
    assert (np.diff(gids)[same] > 0).all(), "compact gids not strictly ascending inside a bin"
    cum = got["cum_tiles_hit"][:V].astype(np.int64)
    hits = np.diff(cum, prepend=0)
    assert (hits >= 0).all()
    counts = np.bincount(gids, minlength=V)
    if got["overflow"]:
        assert (counts <= hits).all(), "a splat has more entries than tiles_hit"
    else:
        assert cum[-1] == I and np.array_equal(counts, hits), "entries per splat differ from the cum_tiles_hit steps"
    bb = BC.reference_bbox(got["projected_splats"][:V], (tbx, tby), np.float32)[gids]
    tx, ty = tile_of % tbx, tile_of // tbx
    inside = (tx >= bb[:, 0]) & (tx < bb[:, 2]) & (ty >= bb[:, 1]) & (ty < bb[:, 3])
    assert inside.all(), f"{int((~inside).sum())} entries lie outside their splat's bbox"
