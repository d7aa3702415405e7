"""An independent restatement of the compressed splat layout (include/brush_hip.h, "compressed splats"): numpy float32
scalars in plain loops, one splat and one operation at a time, nothing shared with brush_amd/compress.py or the
compressed functions of brush_amd/ply.py.  det_expf / det_logf are the oracle's (the library's fixed recipes restated in
C).  tests/test_compress_cpu.py and tests/test_gpu_compress.py compare the product with this, bit for bit."""
import numpy as np

from oracle import oracle as O

F = np.float32
CHUNK = 256
SH_C0 = F(0.28209479177387814)
CHUNK_PROPS = ["min_x", "min_y", "min_z", "max_x", "max_y", "max_z",
               "min_scale_x", "min_scale_y", "min_scale_z", "max_scale_x", "max_scale_y", "max_scale_z",
               "min_r", "min_g", "min_b", "max_r", "max_g", "max_b"]
VERTEX_PROPS = ["packed_position", "packed_rotation", "packed_scale", "packed_color"]


def canon(v):
    """v + 0.0f: -0 becomes +0."""
    return F(v) + F(0.0)


def det_sigmoid(x):
    return F(1.0) / (F(1.0) + F(O.det_expf(float(-F(x)))))


def spread(v):
    """Bit i of the 10-bit v to bit 3 i."""
    out = 0
    for i in range(10):
        out |= ((v >> i) & 1) << (3 * i)
    return out


def norm(v, lo, hi):
    if v <= lo:
        return F(0.0)
    if v >= hi:
        return F(1.0)
    if hi - lo < F(1e-5):
        return F(0.0)
    return (v - lo) / (hi - lo)


def unorm(t, bits):
    top = (1 << bits) - 1
    r = np.floor(F(t) * F(top) + F(0.5))
    if not r > 0:  # negative, zero or NaN
        return 0
    return top if r >= top else int(r)


def morton_keys(means):
    n = means.shape[0]
    pts = [[canon(means[i, k]) for k in range(3)] for i in range(n)]
    finite = [[p[k] for p in pts if not np.isnan(p[k])] for k in range(3)]
    lo = [min(col) if col else F(np.inf) for col in finite]
    hi = [max(col) if col else F(-np.inf) for col in finite]
    keys = []
    for p in pts:
        q = []
        for k in range(3):
            if hi[k] == lo[k]:
                q.append(0)
                continue
            t = ((p[k] - lo[k]) / (hi[k] - lo[k])) * F(1024.0)
            q.append(0 if not t >= 0 else min(1023, int(t)))
        keys.append(spread(q[2]) << 2 | spread(q[1]) << 1 | spread(q[0]))
    return keys


def morton_order(means):
    """Indices of the splats, stably sorted by Morton key (ties keep index order)."""
    keys = morton_keys(np.asarray(means, dtype=F))
    return sorted(range(len(keys)), key=lambda i: keys[i])  # Python's sort is stable


def pack_rotation(rot):
    a = [canon(rot[i]) for i in range(4)]
    length = np.sqrt(((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]) + a[3] * a[3])
    if not length > 0 or not np.isfinite(length):
        a = [F(1.0), F(0.0), F(0.0), F(0.0)]
    else:
        a = [v / length for v in a]
    big = 0
    for i in range(1, 4):
        if abs(a[i]) > abs(a[big]):
            big = i
    if a[big] < 0:
        a = [-v for v in a]
    word = big
    for i in range(4):
        if i != big:
            word = (word << 10) | unorm(a[i] * F(0.70710678) + F(0.5), 10)
    return word


def sh_byte(v):
    r = np.floor((canon(v) / F(8.0) + F(0.5)) * F(256.0))
    if not r > 0:
        return 0
    return 255 if r >= 255 else int(r)


def pack(means, log_scales, rotation, raw_opacity, sh_coeffs, sh_degree=None):
    """dict(order int32 [N], chunks f32 [C,18], words u32 [N,4], sh u8 [N,3K]) of the five float32 arrays of a cloud
    (the Splats layout; sh_coeffs [N,(d+1)^2,3]).  sh_degree: the degree written, at most the input's."""
    means, log_scales, rotation = (np.asarray(a, dtype=F) for a in (means, log_scales, rotation))
    raw_opacity, sh_coeffs = np.asarray(raw_opacity, dtype=F), np.asarray(sh_coeffs, dtype=F)
    n = means.shape[0]
    deg_in = {1: 0, 4: 1, 9: 2, 16: 3}[sh_coeffs.shape[1]]
    deg = deg_in if sh_degree is None else sh_degree
    assert 0 <= deg <= deg_in
    k_out = (deg + 1) ** 2 - 1
    with np.errstate(all="ignore"):
        order = morton_order(means)
        num_chunks = -(-n // CHUNK)
        chunks = np.zeros((num_chunks, 18), dtype=F)
        words = np.zeros((n, 4), dtype=np.uint32)
        sh = np.zeros((n, 3 * k_out), dtype=np.uint8)
        for j in range(num_chunks):
            rows = range(CHUNK * j, min(CHUNK * (j + 1), n))
            quantities = []
            for row in rows:
                g = order[row]
                p = [canon(means[g, k]) for k in range(3)]
                s = [min(max(canon(log_scales[g, k]), F(-20.0)), F(20.0)) for k in range(3)]
                c = [canon(sh_coeffs[g, 0, k]) * SH_C0 + F(0.5) for k in range(3)]
                quantities.append(p + s + c)
            lo = [min(q[k] for q in quantities) for k in range(9)]
            hi = [max(q[k] for q in quantities) for k in range(9)]
            for grp in range(3):
                for k in range(3):
                    chunks[j, 6 * grp + k] = lo[3 * grp + k]
                    chunks[j, 6 * grp + 3 + k] = hi[3 * grp + k]
            for row, q in zip(rows, quantities):
                g = order[row]
                t = [norm(q[k], lo[k], hi[k]) for k in range(9)]
                words[row, 0] = unorm(t[0], 11) << 21 | unorm(t[1], 10) << 11 | unorm(t[2], 11)
                words[row, 1] = pack_rotation(rotation[g])
                words[row, 2] = unorm(t[3], 11) << 21 | unorm(t[4], 10) << 11 | unorm(t[5], 11)
                alpha = det_sigmoid(canon(raw_opacity[g]))
                words[row, 3] = unorm(t[6], 8) << 24 | unorm(t[7], 8) << 16 | unorm(t[8], 8) << 8 | unorm(alpha, 8)
                for c in range(3):
                    for k in range(1, k_out + 1):
                        sh[row, c * k_out + (k - 1)] = sh_byte(sh_coeffs[g, k, c])
    return {"order": np.asarray(order, dtype=np.int32), "chunks": chunks, "words": words, "sh": sh, "sh_degree": deg}


def unpack(chunks, words, sh):
    """dict(means, log_scales, rotation, raw_opacity, sh_coeffs) of packed arrays, rows in packed order."""
    chunks, words, sh = np.asarray(chunks, dtype=F), np.asarray(words).view(np.uint32), np.asarray(sh, dtype=np.uint8)
    n, k_in = words.shape[0], sh.shape[1] // 3
    out = {"means": np.zeros((n, 3), F), "log_scales": np.zeros((n, 3), F), "rotation": np.zeros((n, 4), F),
           "raw_opacity": np.zeros(n, F), "sh_coeffs": np.zeros((n, k_in + 1, 3), F)}

    def lerp(code, bits, lo, hi):
        t = F(code) / F((1 << bits) - 1)
        return lo * (F(1.0) - t) + hi * t

    with np.errstate(all="ignore"):
        for row in range(n):
            ch = chunks[row >> 8]
            for name, word, base in (("means", int(words[row, 0]), 0), ("log_scales", int(words[row, 2]), 6)):
                out[name][row, 0] = lerp(word >> 21, 11, ch[base], ch[base + 3])
                out[name][row, 1] = lerp((word >> 11) & 0x3FF, 10, ch[base + 1], ch[base + 4])
                out[name][row, 2] = lerp(word & 0x7FF, 11, ch[base + 2], ch[base + 5])
            word = int(words[row, 1])
            big = word >> 30
            rest = [(F((word >> shift) & 0x3FF) / F(1023.0) - F(0.5)) * F(1.41421356) for shift in (20, 10, 0)]
            top = np.sqrt(max(F(0.0), F(1.0) - ((rest[0] * rest[0] + rest[1] * rest[1]) + rest[2] * rest[2])))
            others = iter(rest)
            for i in range(4):
                out["rotation"][row, i] = top if i == big else next(others)
            word = int(words[row, 3])
            for c in range(3):
                colour = lerp((word >> (24 - 8 * c)) & 0xFF, 8, ch[12 + c], ch[15 + c])
                out["sh_coeffs"][row, 0, c] = (colour - F(0.5)) / SH_C0
                for k in range(1, k_in + 1):
                    byte = sh[row, c * k_in + (k - 1)]
                    out["sh_coeffs"][row, k, c] = ((F(byte) + F(0.5)) / F(256.0) - F(0.5)) * F(8.0)
            alpha = min(max(F(word & 0xFF), F(0.5)), F(254.5)) / F(255.0)
            out["raw_opacity"][row] = F(O.det_logf(float(alpha / (F(1.0) - alpha))))
    return out


def write_ply(chunks, words, sh) -> bytes:
    """The file of the format text, written without the product's writer: elements chunk, vertex, sh."""
    n = words.shape[0]
    lines = ["ply", "format binary_little_endian 1.0", "comment Exported from Brush", "comment Vertical axis: y",
             f"element chunk {chunks.shape[0]}"] + [f"property float {p}" for p in CHUNK_PROPS]
    lines += [f"element vertex {n}"] + [f"property uint {p}" for p in VERTEX_PROPS]
    if sh.shape[1]:
        lines += [f"element sh {n}"] + [f"property uchar f_rest_{i}" for i in range(sh.shape[1])]
    lines.append("end_header")
    body = np.asarray(chunks, "<f4").tobytes() + np.asarray(words, "<u4").tobytes() + np.asarray(sh, np.uint8).tobytes()
    return ("\n".join(lines) + "\n").encode("ascii") + body
