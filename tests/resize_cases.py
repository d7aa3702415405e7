"""Directed shapes for the area-filter tests: one case per side of every switch in brush_amd/csrc/resize.hip.

brush_area_resize_u8 picks its code path from the shapes alone.  `regime` restates that choice (the host code of the
entry point, and the quantities every workgroup of k_area_resize / k_area_resize_int derives from its block index) in
plain Python; it is used ONLY to assert that a case sits where its name says, never for correctness.  `CASES` names the
shapes, `image` builds the patterns every case is run on, `block_sum_image` the sources of the integer kernel's
block-sum sweep.  Plain numpy; nothing here needs a GPU.  When a constant below is retuned in resize.hip,
tests/test_pyramid_cpu.py::test_every_case_sits_in_the_regime_it_names says which case has to move.
"""
import numpy as np

THREADS = 256            # kThreads
WAVE = 64                # kWave
MIN_LDS_VECS = 64        # kMinLdsVecs
MAX_LDS_VECS = 2048      # kMaxLdsVecs
MAX_BATCH_ROWS = 16      # kMaxBatchRows
MAX_STRIP_ROWS = 8       # kMaxStripRows
WANT_WORKGROUPS = 2048   # kWantWorkgroups
FEW_WORKGROUPS = 1024    # kFewWorkgroups
MAX_INT_BLOCK = 256      # kMaxIntBlock


def _ceil_div(a, b):
    return (a + b - 1) // b


def regime(w, h, ow, oh, channels):
    """The path brush_area_resize_u8 takes for a [h,w,channels] source and an [oh,ow] output, as a dict.

    Both kernels: kernel ("int" | "general"), threads, workgroups (x, y), lds_vecs, live_last (live lanes of the last
    column group), and per column group, as a (first, last) pair: slot, batch.
    general: wide, strip_rows, ragged (the last strip is shorter), and pairs fits, chunks (per source row);
             source_rows is the (first, last) strip's count of source rows.
    int:     fx, fy and the pair rounds (barrier rounds over the fy source rows)."""
    assert 1 <= ow <= w <= 16384 and 1 <= oh <= h <= 16384 and channels in (3, 4)
    threads = WAVE if _ceil_div(ow, THREADS) * oh < FEW_WORKGROUPS else THREADS
    col_groups = _ceil_div(ow, threads)
    groups = [(g * threads, min((g + 1) * threads, ow)) for g in (0, col_groups - 1)]
    out = dict(threads=threads, live_last=groups[1][1] - groups[1][0])
    fx, fy = w // ow, h // oh
    int_slot = (threads * fx * channels + 15) // 16 + 1
    if fx * ow == w and fy * oh == h and fx * fy <= MAX_INT_BLOCK and int_slot <= MAX_LDS_VECS:
        lds = min(max(int_slot * min(fy, MAX_BATCH_ROWS), MIN_LDS_VECS), MAX_LDS_VECS)
        slot = tuple(((x1 - x0) * fx * channels + 15) // 16 + 1 for x0, x1 in groups)
        batch = tuple(min(lds // s, MAX_BATCH_ROWS) for s in slot)
        assert all(b >= 1 for b in batch)
        out.update(kernel="int", workgroups=(col_groups, oh), lds_vecs=lds, fx=fx, fy=fy, slot=slot, batch=batch,
                   rounds=tuple(_ceil_div(fy, b) for b in batch))
        return out
    strip_rows = min(max(oh * col_groups // WANT_WORKGROUPS, 1), MAX_STRIP_ROWS)
    strips = _ceil_div(oh, strip_rows)
    host_slot = ((threads * w // ow + 2) * channels + 15) // 16 + 1
    rows = min(strip_rows * h // oh + 2, MAX_BATCH_ROWS)
    lds = min(max(host_slot * rows, MIN_LDS_VECS), MAX_LDS_VECS)
    D = w * h
    slot, fits, batch, chunks = [], [], [], []
    for x0, x1 in groups:
        c_lo, c_hi = x0 * w // ow, (x1 * w - 1) // ow + 1
        s = ((c_hi - c_lo) * channels + 15) // 16 + 1
        f = s <= lds
        chunk_cols = c_hi - c_lo if f else (lds * 16 - 32) // channels
        slot.append(s), fits.append(f), batch.append(min(lds // s, MAX_BATCH_ROWS) if f else 1)
        chunks.append(_ceil_div(c_hi - c_lo, chunk_cols))
    source_rows = []
    for y0 in (0, (strips - 1) * strip_rows):
        y1 = min(y0 + strip_rows, oh)
        source_rows.append((y1 * h - 1) // oh + 1 - y0 * h // oh)
    out.update(kernel="general", workgroups=(col_groups, strips), lds_vecs=lds, wide=255 * D + D // 2 >= 1 << 32,
               strip_rows=strip_rows, ragged=oh % strip_rows != 0, slot=tuple(slot), fits=tuple(fits),
               batch=tuple(batch), chunks=tuple(chunks), source_rows=tuple(source_rows))
    return out


# name -> (w, h, ow, oh, fields for both channel counts, fields for RGB only, fields for RGBA only).  A pair is (first,
# last) column group or strip, as `regime` returns it.
_G64, _G256 = dict(kernel="general", threads=64), dict(kernel="general", threads=256)
_I64, _I256 = dict(kernel="int", threads=64), dict(kernel="int", threads=256)
_CHUNKS2, _CHUNKS3 = dict(fits=(False, False), chunks=(2, 2)), dict(fits=(False, False), chunks=(3, 3))
_WHOLE = dict(fits=(True, True), chunks=(1, 1))
CASES = {
    # 64 / 256 lanes: ceil(ow / 256) oh against kFewWorkgroups
    "lanes_64_at_1023": (40, 1100, 33, 1023, dict(_G64, workgroups=(1, 1023), strip_rows=1, **_WHOLE), {}, {}),
    "lanes_256_at_1024": (40, 1100, 33, 1024, dict(_G256, workgroups=(1, 1024), strip_rows=1, **_WHOLE), {}, {}),
    "small_general": (130, 100, 43, 33, dict(_G64, wide=False, strip_rows=1, batch=(7, 7), **_WHOLE), {}, {}),
    # the path of a 1920 x 1080 training image at a non-integer ratio
    "workload_1080p": (1920, 1080, 1280, 720, dict(_G256, wide=False, strip_rows=1, live_last=256, batch=(3, 3),
                                                   source_rows=(2, 2), **_WHOLE), {}, {}),
    # strips of 2, 3, 7, 8 output rows: oh col_groups / kWantWorkgroups, capped at kMaxStripRows
    "strip_2": (260, 2100, 257, 2048, dict(_G256, strip_rows=2, ragged=False, live_last=1, source_rows=(3, 3)), {}, {}),
    "strip_2_ragged": (260, 3100, 257, 3071, dict(_G256, strip_rows=2, ragged=True, live_last=1, source_rows=(3, 2)), {}, {}),
    "strip_3": (260, 3100, 257, 3072, dict(_G256, strip_rows=3, ragged=False, live_last=1, source_rows=(4, 4)), {}, {}),
    "strip_7_ragged": (260, 8300, 257, 8191, dict(_G256, strip_rows=7, ragged=True, live_last=1, source_rows=(8, 2)), {}, {}),
    "strip_8": (260, 8300, 257, 8192, dict(_G256, strip_rows=8, ragged=False, live_last=1, source_rows=(9, 9)), {}, {}),
    "strip_8_capped_ragged": (260, 16384, 257, 16383, dict(_G256, strip_rows=8, ragged=True, live_last=1,
                                                           workgroups=(2, 2048), source_rows=(9, 8)), {}, {}),
    # one row in chunks, every lane live (a lane's taps lie in one chunk, or straddle two)
    "chunked_64_lanes": (16384, 3, 64, 3, dict(_G64, live_last=64, batch=(1, 1), source_rows=(1, 1)), _CHUNKS2, _CHUNKS3),
    "chunked_63_lanes": (16384, 3, 63, 2, dict(_G64, live_last=63, batch=(1, 1), source_rows=(2, 2)), _CHUNKS2, _CHUNKS3),
    # 256 lanes: int_slot against kMaxLdsVecs, and chunking
    "fx31_256_lanes": (7936, 1024, 256, 1024, dict(_I256, fx=31, fy=1, rounds=(1, 1)),
                       dict(slot=(1489, 1489)), dict(slot=(1985, 1985))),
    "fx32_256_lanes": (8192, 1024, 256, 1024, dict(threads=256, live_last=256),
                       dict(kernel="int", fx=32, slot=(1537, 1537)), dict(kernel="general", source_rows=(1, 1), **_CHUNKS2)),
    "chunked_256_lanes": (8191, 1030, 255, 1024, dict(_G256, live_last=255, batch=(1, 1), source_rows=(2, 2)),
                          dict(slot=(1537, 1537), **_WHOLE), dict(slot=(2049, 2049), **_CHUNKS2)),
    # 64 lanes: int_slot against kMaxLdsVecs, one source row per barrier round
    "fx127_64_lanes": (8128, 2, 64, 1, dict(_I64, fx=127, fy=2, batch=(1, 1), rounds=(2, 2)),
                       dict(slot=(1525, 1525)), dict(slot=(2033, 2033))),
    "fx128_64_lanes": (8192, 2, 64, 1, dict(threads=64, live_last=64),
                       dict(kernel="int", fx=128, slot=(1537, 1537), rounds=(2, 2)), dict(kernel="general", **_CHUNKS2)),
    "fx85_batch_2_or_1": (5440, 4, 64, 2, dict(_I64, fx=85, fy=2),
                          dict(batch=(2, 2), rounds=(1, 1)), dict(batch=(1, 1), rounds=(2, 2))),
    # the integer kernel over several barrier rounds: fy above kMaxBatchRows
    "fy17_two_rounds": (60, 68, 60, 4, dict(_I64, fx=1, fy=17, batch=(16, 16), rounds=(2, 2)), {}, {}),
    "15x17_two_rounds": (15, 34, 1, 2, dict(_I64, fx=15, fy=17, batch=(16, 16), rounds=(2, 2)), {}, {}),
    "fy255_16_rounds": (1, 255, 1, 1, dict(_I64, fx=1, fy=255, batch=(16, 16), rounds=(16, 16)), {}, {}),
    # fx fy against kMaxIntBlock
    "block_256_square": (16, 16, 1, 1, dict(_I64, fx=16, fy=16, rounds=(1, 1)), {}, {}),
    "block_256_flat": (32, 8, 1, 1, dict(_I64, fx=32, fy=8, rounds=(1, 1)), {}, {}),
    "block_272": (17, 16, 1, 1, dict(_G64, source_rows=(16, 16), **_WHOLE), {}, {}),
    "block_1024": (128, 128, 4, 4, dict(_G64, source_rows=(32, 32), **_WHOLE), {}, {}),
    # extreme sides
    "identity_row": (16384, 1, 16384, 1, dict(_I64, fx=1, fy=1, workgroups=(256, 1)), {}, {}),
    "row_to_pixel": (16384, 1, 1, 1, dict(_G64, live_last=1, source_rows=(1, 1)), _CHUNKS2, _CHUNKS3),
    "column_to_pixel": (1, 16384, 1, 1, dict(_G64, source_rows=(16384, 16384), batch=(16, 16), **_WHOLE), {}, {}),
    "identity_column": (1, 16384, 1, 16384, dict(_I256, fx=1, fy=1, workgroups=(1, 16384)), {}, {}),
    "row_16384_to_16383": (16384, 2, 16383, 1, dict(_G64, workgroups=(256, 1), live_last=63, source_rows=(2, 2), **_WHOLE), {}, {}),
}
# The accumulator switch, 255 D + D // 2 against 2^32, depends on D = w h alone: 16384 x 1026 is the largest D below it
# (the `full` image takes the 32-bit accumulator to 4 294 950 912), 16384 x 1027 the first above.  RGB only; the images
# are tests/test_gpu_resize_regimes.py's (test_accumulator_switch_equals_the_reference).
LARGE_CASES = {
    "acc32_strips_of_8": (16384, 1026, 8191, 513, dict(_G256, wide=False, strip_rows=8, ragged=True, source_rows=(16, 2),
                                                       **_WHOLE), {}, {}),
    "acc32_chunked": (16384, 1026, 3, 2, dict(_G64, wide=False, source_rows=(513, 513)), _CHUNKS2, {}),
    "acc64_strips_of_8": (16384, 1027, 8191, 513, dict(_G256, wide=True, strip_rows=8, ragged=True, source_rows=(17, 3),
                                                       **_WHOLE), {}, {}),
    "acc64_chunked": (16384, 1027, 3, 2, dict(_G64, wide=True, source_rows=(514, 514)), _CHUNKS2, {}),
}
PATTERNS = ("random", "zeros", "full", "ramp", "coin", "coin254")
# Exact ties of the `coin` image, S mod D == D // 2 with D even, per case of CASES as (RGB, RGBA): the outputs whose value is the
# rounding rule's alone (counted by `tie_count`; tests/test_pyramid_cpu.py recounts the cases of up to 2^20 pixels,
# tests/test_gpu_resize_regimes.py all of them).
TIES = {
    "lanes_64_at_1023": (961, 1375), "lanes_256_at_1024": (777, 997), "small_general": (3, 8), "workload_1080p": (0, 0),
    "strip_2": (1583, 2070), "strip_2_ragged": (2487, 3292), "strip_3": (2369, 3080), "strip_7_ragged": (6427, 8463),
    "strip_8": (6119, 8278), "strip_8_capped_ragged": (12439, 16846), "chunked_64_lanes": (21, 32), "chunked_63_lanes": (0, 0),
    "fx31_256_lanes": (0, 0), "fx32_256_lanes": (110410, 146118), "chunked_256_lanes": (0, 0), "fx127_64_lanes": (10, 8),
    "fx128_64_lanes": (10, 14), "fx85_batch_2_or_1": (22, 28), "fy17_two_rounds": (0, 0), "15x17_two_rounds": (0, 0),
    "fy255_16_rounds": (0, 0), "block_256_square": (0, 0), "block_256_flat": (0, 0), "block_272": (0, 0),
    "block_1024": (0, 0), "identity_row": (0, 0), "row_to_pixel": (0, 0), "column_to_pixel": (0, 0),
    "identity_column": (0, 0), "row_16384_to_16383": (12406, 16569),
}


def expected(name, channels):
    """(w, h, ow, oh, the regime fields the case names for this channel count)."""
    w, h, ow, oh, both, rgb, rgba = {**CASES, **LARGE_CASES}[name]
    return w, h, ow, oh, {**both, **(rgb if channels == 3 else rgba)}


def seed_of(name, channels):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) * 10 + channels


def image(w, h, channels, pattern, seed):
    """A uint8 [h,w,channels] test image.  random, zeros, full and ramp are test_gpu_pyramid._patterns' (the ramp in
    wrapping uint8 sums: the same bytes); coin is 0 or 1 with probability 1/2 per byte, so that every output is a
    rounding decision at D / 2; coin254 is coin + 254, the same decisions at the top of the range."""
    shape = (h, w, channels)
    if pattern == "random":
        return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)
    if pattern == "zeros":
        return np.zeros(shape, np.uint8)
    if pattern == "full":
        return np.full(shape, 255, np.uint8)
    if pattern == "ramp":
        r, s, c = ((np.arange(n) * k % 256).astype(np.uint8) for n, k in ((h, 7), (w, 3), (channels, 50)))
        return r[:, None, None] + s[None, :, None] + c[None, None, :]
    coin = np.random.default_rng(seed + 1).integers(0, 2, shape, dtype=np.uint8)
    if pattern == "coin":
        return coin
    assert pattern == "coin254"
    return coin + np.uint8(254)


def tie_count(S, D):
    """Outputs of the weighted sums S (pyramid_ref.area_sums_integral) that sit exactly between two bytes."""
    return int((S % D == D // 2).sum()) if D % 2 == 0 else 0


# ---- the integer kernel's division, on every sum it can see ----------------------------------------------------------
# (fx, fy, (ow, oh) that launches 64 lanes, (ow, oh) that launches 256 lanes or None).  ow oh >= 255 fx fy + 1 blocks,
# sides within 16384, at most 51 MB as RGB.  No 256-lane shape exists within 70 MB for three of them: 256 lanes need
# ceil(ow / 256) oh >= 1024, which at fy = 17 (oh <= 963) takes 257 x 512 blocks (100 MB) and at fy = 255 (oh <= 64)
# 3841 x 64 blocks (188 MB); at fx = 127, 256 lanes' rows exceed the staging buffer and the general kernel takes over.
SWEEP = [
    (1, 1, (16, 17), (1, 1024)),
    (2, 1, (23, 23), (1, 1024)),
    (1, 3, (28, 28), (1, 1024)),
    (3, 3, (48, 48), (3, 1024)),
    (5, 3, (62, 62), (4, 1024)),
    (15, 17, (255, 256), None),
    (16, 16, (256, 256), (64, 1024)),
    (32, 8, (256, 256), (64, 1024)),
    (1, 255, (1017, 64), None),
    (127, 2, (129, 503), None),
]


def block_sum_image(fx, fy, ow, oh, channels=3, seed=0, blocks=None):
    """A uint8 [fy oh, fx ow, channels] image whose fy x fx blocks have, per channel, every sum 0 .. 255 fx fy (block i
    of the channel holds sum perm[i mod B], perm a seeded shuffle of the B = 255 fx fy + 1 sums; ow oh >= B), each
    block's bytes filled greedily: 255s, one remainder, zeros.  Returns (image, the blocks' sums [oh,ow,channels],
    blocks); `blocks` can be handed to a call for another ow x oh of as many blocks, which then lays out the same ones."""
    n, count = fx * fy, ow * oh
    B = 255 * n + 1
    assert count >= B
    if blocks is None or blocks[0].shape[0] != count:
        rng = np.random.default_rng(seed + 1000 * fx + fy)
        fill = np.arange(B, dtype=np.int32)[:, None] - 255 * np.arange(n, dtype=np.int32)[None, :]
        by_sum = np.clip(fill, 0, 255, out=fill).astype(np.uint8)  # [B, n]: row k is the block of sum k
        sums = np.stack([rng.permutation(B)[np.arange(count) % B] for _ in range(channels)], axis=1)
        blocks = sums, np.stack([by_sum[sums[:, c]] for c in range(channels)], axis=2)  # [count, n, channels]
    sums, vals = blocks
    img = vals.reshape(oh, ow, fy, fx, channels).transpose(0, 2, 1, 3, 4).reshape(fy * oh, fx * ow, channels)
    return np.ascontiguousarray(img), sums.reshape(oh, ow, channels), blocks
