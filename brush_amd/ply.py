"""Inria-layout splat PLY import / export — host-side numpy, not on the hot path.

Mirrors crates/brush-dataset/src/splat_import.rs:168-312 (ASCII / binary LE / binary BE, required
properties, `f_rest_*` channel-major de-interleave, truncation to SH degree 3) and
crates/brush-dataset/src/splat_export.rs:11-106 (property order, comments, binary little endian).
`scale_*` are log-scales, `opacity` is the raw (pre-sigmoid) value, `rot_*` is (w, x, y, z).

Build extension: the chunk-quantised "compressed PLY" layout (elements `chunk`, `vertex` with four packed words, `sh`
bytes; include/brush_hip.h states every word).  `compressed_to_ply` / `load_compressed_ply` move the packed arrays,
which the device kernels of brush_amd/compress.py produce and consume; `load_splat_from_ply` unpacks such a file in
numpy, so that it reads on a machine without a GPU.
"""
from __future__ import annotations

import io

import numpy as np

_PLY_TYPES = {
    "char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
    "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
    "double": "f8", "float64": "f8",
}
_MIN_PROPS = ["x", "y", "z", "scale_0", "scale_1", "scale_2", "opacity", "rot_0", "rot_1", "rot_2", "rot_3",
              "f_dc_0", "f_dc_1", "f_dc_2"]  # splat_import.rs:198-202
_MAX_SH_COEFFS = 16  # "Limit the number of imported SH channels for now" (splat_import.rs:241-246)


def _parse_header(buf: bytes):
    end = buf.find(b"end_header")
    if end < 0 or not buf.startswith(b"ply"):
        raise ValueError("Invalid ply file")
    nl = buf.find(b"\n", end)
    lines = buf[:end].decode("ascii", "replace").splitlines()
    fmt, elements, cur = None, [], None
    for ln in lines[1:]:
        t = ln.split()
        if not t or t[0] == "comment":
            continue
        if t[0] == "format":
            fmt = t[1]
        elif t[0] == "element":
            cur = {"name": t[1], "count": int(t[2]), "props": []}
            elements.append(cur)
        elif t[0] == "property":
            if t[1] == "list":
                raise ValueError("list properties are not supported in splat ply files")
            cur["props"].append((t[2], _PLY_TYPES[t[1]]))
    if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
        raise ValueError(f"Invalid ply format {fmt}")
    return fmt, elements, nl + 1


def _read_bytes(data) -> bytes:
    if isinstance(data, (bytes, bytearray)):
        return bytes(data)
    with open(data, "rb") as f:
        return f.read()


def load_splat_from_ply(data) -> dict:
    """Returns dict(means[N,3], log_scales[N,3], rotation[N,4], raw_opacity[N], sh_coeffs[N,C,3]) f32.

    A compressed PLY (is_compressed_ply) is unpacked in numpy (unpack_compressed), rows in the file's order.  Every
    value is then the bits brush_splat_unpack gives on the device, except raw_opacity: numpy's float64 log rounded to
    float32 stands in for the device's fixed-recipe det_logf (2 ulp), so the two may differ by a few ulp (at most 3)."""
    data = _read_bytes(data)
    fmt, elements, off = _parse_header(data)
    if _is_compressed(elements):
        return unpack_compressed(*load_compressed_ply(data))
    verts = None
    for el in elements:
        names = [p[0] for p in el["props"]]
        if fmt == "ascii":
            txt = io.BytesIO(data[off:])
            arr = np.loadtxt(txt, dtype=np.float64, max_rows=el["count"], ndmin=2) if el["count"] else np.zeros((0, len(names)))
            consumed = sum(len(l) for l in data[off:].splitlines(keepends=True)[: el["count"]])
            table = {n: arr[:, i] for i, n in enumerate(names)}
            off += consumed
        else:
            e = "<" if fmt == "binary_little_endian" else ">"
            dt = np.dtype([(n, e + t) for n, t in el["props"]])
            arr = np.frombuffer(data, dtype=dt, count=el["count"], offset=off)
            table = {n: arr[n] for n in names}
            off += dt.itemsize * el["count"]
        if el["name"] == "vertex":
            verts = table
    if verts is None:
        raise ValueError("Invalid ply file")
    if not all(p in verts for p in _MIN_PROPS):
        raise ValueError("Invalid splat ply. Missing properties!")

    def col(*names):
        return np.stack([np.asarray(verts[n], dtype=np.float32) for n in names], axis=1)

    n = len(verts["x"])
    if n == 0:
        raise ValueError("No splats found")
    rest_ids = sorted(int(k[len("f_rest_"):]) for k in verts if k.startswith("f_rest_") and k[len("f_rest_"):].isdigit())
    n_rest = (max(rest_ids) + 1) if rest_ids else 0
    dc = col("f_dc_0", "f_dc_1", "f_dc_2")  # [N,3]
    if n_rest:
        rest = col(*[f"f_rest_{i}" for i in range(n_rest)])  # channel-major: [R.., G.., B..]
        cpc = n_rest // 3
        rest = rest[:, : cpc * 3].reshape(n, 3, cpc).transpose(0, 2, 1)  # interleave_coeffs -> [N, cpc, 3]
        sh = np.concatenate([dc[:, None, :], rest], axis=1)
    else:
        sh = dc[:, None, :]
    sh = sh[:, :_MAX_SH_COEFFS]
    return {
        "means": col("x", "y", "z"),
        "log_scales": col("scale_0", "scale_1", "scale_2"),
        "rotation": col("rot_0", "rot_1", "rot_2", "rot_3"),
        "raw_opacity": np.asarray(verts["opacity"], dtype=np.float32).copy(),
        "sh_coeffs": np.ascontiguousarray(sh, dtype=np.float32),
    }


def splat_to_ply(means, log_scales, rotation, raw_opacity, sh_coeffs) -> bytes:
    """Binary little-endian PLY in the reference's property order (splat_export.rs:67-105)."""
    means = np.asarray(means, np.float32)
    n, c = means.shape[0], np.asarray(sh_coeffs).shape[1]
    sh = np.asarray(sh_coeffs, np.float32).transpose(0, 2, 1)  # Inria layout [n, channel, coeffs]
    dc = sh[:, :, 0]
    rest = sh[:, :, 1:].reshape(n, 3 * (c - 1))
    names = list(_MIN_PROPS) + [f"f_rest_{i}" for i in range(3 * (c - 1))]
    cols = np.concatenate([means, np.asarray(log_scales, np.float32), np.asarray(raw_opacity, np.float32)[:, None],
                           np.asarray(rotation, np.float32), dc, rest], axis=1).astype("<f4")
    header = ["ply", "format binary_little_endian 1.0", "comment Exported from Brush", "comment Vertical axis: y",
              f"element vertex {n}"] + [f"property float {nm}" for nm in names] + ["end_header"]
    return ("\n".join(header) + "\n").encode("ascii") + np.ascontiguousarray(cols).tobytes()


# ---------------------------------------------------------------------------- compressed PLY (build extension)
CHUNK = 256  # rows of a chunk (BRUSH_SPLAT_CHUNK)
_CHUNK_PROPS = ["min_x", "min_y", "min_z", "max_x", "max_y", "max_z",
                "min_scale_x", "min_scale_y", "min_scale_z", "max_scale_x", "max_scale_y", "max_scale_z",
                "min_r", "min_g", "min_b", "max_r", "max_g", "max_b"]
_PACKED_PROPS = ["packed_position", "packed_rotation", "packed_scale", "packed_color"]
_SH_REST = {0: 0, 3: 1, 8: 2, 15: 3}  # higher-order coefficients per channel -> SH degree
SH_C0 = np.float32(0.28209479177387814)


def sh_rest_count(sh_degree: int) -> int:
    """K: the higher-order SH coefficients per channel of a degree the compressed layout has (0..3)."""
    if sh_degree not in (0, 1, 2, 3):
        raise ValueError(f"the compressed layout holds SH degrees 0 to 3, got {sh_degree}")
    return (sh_degree + 1) ** 2 - 1


def _is_compressed(elements) -> bool:
    by_name = {el["name"]: [p[0] for p in el["props"]] for el in elements}
    return "chunk" in by_name and all(p in by_name.get("vertex", ()) for p in _PACKED_PROPS)


def is_compressed_ply(data) -> bool:
    """True when `data` (a path or bytes) is a PLY in the compressed layout: a `chunk` element and a `vertex` element
    that holds the four packed words.  False for any other PLY; ValueError for what is no PLY at all."""
    return _is_compressed(_parse_header(_read_bytes(data))[1])


def load_compressed_ply(data):
    """(chunks f32 [C,18], words u32 [N,4], sh u8 [N,3K]) of a compressed PLY (a path or bytes), K = 0 without an `sh`
    element.  ValueError for another layout, an ASCII file, counts that do not belong together (C = ceil(N / 256), one
    `sh` row per vertex) or a coefficient count other than 3 K = 9, 24, 45."""
    data = _read_bytes(data)
    fmt, elements, off = _parse_header(data)
    if not _is_compressed(elements):
        raise ValueError("not a compressed splat ply: it needs a `chunk` element and packed vertex words")
    if fmt == "ascii":
        raise ValueError("a compressed splat ply must be binary")
    e = "<" if fmt == "binary_little_endian" else ">"
    tables = {}
    for el in elements:
        dt = np.dtype([(n, e + t) for n, t in el["props"]])
        if off + dt.itemsize * el["count"] > len(data):
            raise ValueError(f"the ply ends inside its `{el['name']}` element")
        tables[el["name"]] = np.frombuffer(data, dtype=dt, count=el["count"], offset=off)
        off += dt.itemsize * el["count"]
    chunk, vert = tables["chunk"], tables["vertex"]
    if not all(p in (chunk.dtype.names or ()) for p in _CHUNK_PROPS):
        raise ValueError("Invalid compressed splat ply. Missing chunk properties!")
    n = len(vert)
    if n == 0:
        raise ValueError("No splats found")
    if len(chunk) != -(-n // CHUNK):
        raise ValueError(f"{n} splats need {-(-n // CHUNK)} chunks, the file has {len(chunk)}")
    chunks = np.stack([chunk[p].astype(np.float32) for p in _CHUNK_PROPS], axis=1)
    words = np.stack([vert[p].astype(np.uint32) for p in _PACKED_PROPS], axis=1)
    if "sh" in tables and len(tables["sh"].dtype.names or ()):
        rest = tables["sh"]
        count = len(rest.dtype.names)
        names = [f"f_rest_{i}" for i in range(count)]
        if count % 3 or count // 3 not in _SH_REST or count == 0 or not all(p in rest.dtype.names for p in names):
            raise ValueError(f"a compressed splat ply holds 9, 24 or 45 f_rest_* bytes per splat, got {count}")
        if len(rest) != n:
            raise ValueError(f"the `sh` element has {len(rest)} rows for {n} splats")
        sh = np.stack([rest[p].astype(np.uint8) for p in names], axis=1)
    else:
        sh = np.zeros((n, 0), dtype=np.uint8)
    return np.ascontiguousarray(chunks), np.ascontiguousarray(words), np.ascontiguousarray(sh)


def compressed_to_ply(chunks, words, sh) -> bytes:
    """Binary little-endian compressed PLY of packed arrays: chunks f32 [C,18], words 32-bit [N,4], sh u8 [N,3K]
    (3K = 0, 9, 24 or 45; the `sh` element is absent at 0).  Elements `chunk`, `vertex`, `sh`, in this order."""
    chunks = np.ascontiguousarray(chunks, dtype="<f4")
    words = np.asarray(words)
    if words.dtype.kind not in "iu" or words.dtype.itemsize != 4:
        raise ValueError(f"the packed words must be 32-bit integers, got {words.dtype}")
    words = np.ascontiguousarray(words).view(np.uint32).astype("<u4")
    sh = np.ascontiguousarray(sh, dtype=np.uint8)
    n = words.shape[0]
    if words.ndim != 2 or words.shape[1] != 4 or n == 0:
        raise ValueError(f"the packed words must be [N,4] with N > 0, got {words.shape}")
    if chunks.shape != (-(-n // CHUNK), 18):
        raise ValueError(f"{n} splats need chunks of shape {(-(-n // CHUNK), 18)}, got {chunks.shape}")
    if sh.ndim != 2 or sh.shape[0] != n or sh.shape[1] % 3 or sh.shape[1] // 3 not in _SH_REST:
        raise ValueError(f"the SH bytes must be [{n}, 0 | 9 | 24 | 45], got {sh.shape}")
    header = ["ply", "format binary_little_endian 1.0", "comment Exported from Brush", "comment Vertical axis: y",
              f"element chunk {chunks.shape[0]}"] + [f"property float {p}" for p in _CHUNK_PROPS] + \
             [f"element vertex {n}"] + [f"property uint {p}" for p in _PACKED_PROPS]
    if sh.shape[1]:
        header += [f"element sh {n}"] + [f"property uchar f_rest_{i}" for i in range(sh.shape[1])]
    header.append("end_header")
    return ("\n".join(header) + "\n").encode("ascii") + chunks.tobytes() + words.tobytes() + sh.tobytes()


def _raw_opacity_table() -> np.ndarray:
    """raw_opacity of the 256 opacity codes: the float32 quotient a / (1 - a), a = clamp(code, 0.5, 254.5) / 255, then
    the float64 log rounded to float32 (the device takes det_logf of the same quotient)."""
    code = np.arange(256, dtype=np.float32)
    a = np.minimum(np.maximum(code, np.float32(0.5)), np.float32(254.5)) / np.float32(255.0)
    ratio = a / (np.float32(1.0) - a)
    return np.log(ratio.astype(np.float64)).astype(np.float32)


def unpack_compressed(chunks, words, sh) -> dict:
    """The dict of load_splat_from_ply from packed arrays, in float32 numpy, operation for operation what
    brush_splat_unpack computes (include/brush_hip.h) except the logarithm of the opacity (see load_splat_from_ply)."""
    f = np.float32
    chunks = np.asarray(chunks, dtype=np.float32)
    words = np.ascontiguousarray(words).view(np.uint32)
    sh = np.asarray(sh, dtype=np.uint8)
    n = words.shape[0]
    k = sh.shape[1] // 3
    if sh.shape[1] % 3 or k not in _SH_REST:
        raise ValueError(f"the SH bytes must be [{n}, 0 | 9 | 24 | 45], got {sh.shape}")
    ch = chunks[np.arange(n) >> 8]  # the chunk record of every row

    def lerp(code, bits, lo, hi):
        t = code.astype(f) / f((1 << bits) - 1)
        return lo * (f(1.0) - t) + hi * t

    def triple(w, col):  # 11-10-11 over the chunk columns col..col+2 (min) and col+3..col+5 (max)
        return np.stack([lerp(w >> 21, 11, ch[:, col], ch[:, col + 3]),
                         lerp((w >> 11) & 0x3FF, 10, ch[:, col + 1], ch[:, col + 4]),
                         lerp(w & 0x7FF, 11, ch[:, col + 2], ch[:, col + 5])], axis=1)

    means, log_scales = triple(words[:, 0], 0), triple(words[:, 2], 6)
    rot_w = words[:, 1]
    rest = [((((rot_w >> (10 * (2 - i))) & 0x3FF).astype(f) / f(1023.0)) - f(0.5)) * f(1.41421356) for i in range(3)]
    sumsq = (rest[0] * rest[0] + rest[1] * rest[1]) + rest[2] * rest[2]
    top = np.sqrt(np.maximum(f(0.0), f(1.0) - sumsq))
    big = (rot_w >> 30).astype(np.int64)
    rotation = np.empty((n, 4), dtype=f)
    for i in range(4):
        j = np.where(i < big, i, i - 1)  # which stored component index i holds when it is not the largest
        stored = np.choose(np.clip(j, 0, 2), rest)
        rotation[:, i] = np.where(big == i, top, stored)
    col = words[:, 3]
    dc = np.stack([(lerp((col >> (24 - 8 * c)) & 0xFF, 8, ch[:, 12 + c], ch[:, 15 + c]) - f(0.5)) / SH_C0
                   for c in range(3)], axis=1)
    coeffs = np.empty((n, k + 1, 3), dtype=f)
    coeffs[:, 0, :] = dc
    if k:
        vals = ((sh.astype(f) + f(0.5)) / f(256.0) - f(0.5)) * f(8.0)  # [n, 3k], channel-major
        coeffs[:, 1:, :] = vals.reshape(n, 3, k).transpose(0, 2, 1)
    return {"means": means.astype(f), "log_scales": log_scales.astype(f), "rotation": rotation,
            "raw_opacity": _raw_opacity_table()[col & 0xFF], "sh_coeffs": np.ascontiguousarray(coeffs)}
