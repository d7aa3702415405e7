"""CPU-side checks: the C-ABI library loads and exports every symbol of include/brush_hip.h,
argument validation works without a GPU, host camera/uniform packing mirrors camera.rs."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as G

    if not os.path.exists(os.path.join(ROOT, "brush_amd", "lib", "libbrush_hip.so")):
        G.build()
    from brush_amd import _lib

    return _lib.lib()


def test_library_exports_every_declared_symbol(lib):
    hdr = open(os.path.join(ROOT, "include", "brush_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = sorted(set(re.findall(r"\b(brush_[a-z0-9_]+)\s*\(", hdr)))
    assert len(declared) >= 12
    from brush_amd import _lib

    assert sorted(_lib.SYMBOL_NAMES) == declared
    for name in declared:
        assert hasattr(lib, name), name
    assert b"gfx950" in lib.brush_version()


def test_integration_doc_matches_header():
    """INTEGRATION.md's Rust FFI block is generated from include/brush_hip.h: regenerate and compare
    (symbol set, arity and types), and hold the ctypes binding to the same arity per symbol."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("gen_rust_ffi", os.path.join(ROOT, "tools", "gen_rust_ffi.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    hdr = open(os.path.join(ROOT, "include", "brush_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    block = doc[doc.index(gen.BEGIN) + len(gen.BEGIN):doc.index(gen.END)].strip()
    assert block == gen.generate(hdr).strip(), "run `python tools/gen_rust_ffi.py --write`"
    # no second, hand-written extern block that could drift
    assert doc.count('extern "C" {') == 1
    structs, funcs = gen.parse_header(hdr)
    from brush_amd import _lib

    bound = {name: (restype, argtypes) for name, restype, argtypes in _lib._SYMBOLS}
    assert sorted(bound) == sorted(f[0] for f in funcs)
    for name, ret, params in funcs:
        restype, argtypes = bound[name]
        assert len(argtypes) == len(params), name
        assert (restype is None) == (ret == "void"), name
        for (pname, rtype), ct in zip(params, argtypes):
            is_ptr = rtype.startswith("*")
            ct_ptr = ct is C.c_void_p or ct is C.c_char_p or hasattr(ct, "contents")
            assert is_ptr == bool(ct_ptr), f"{name}.{pname}: {rtype} vs {ct}"
            if not is_ptr:
                want = {"u32": C.c_uint32, "i32": C.c_int, "f32": C.c_float, "usize": C.c_size_t}[rtype]
                assert ct is want, f"{name}.{pname}: {rtype} vs {ct}"
    for sname, fields in structs:
        cs = getattr(_lib, sname)
        assert [f[0] for f in cs._fields_] == [f[0] for f in fields], sname


def test_argument_validation_without_gpu(lib):
    from brush_amd import _lib

    n = C.c_size_t()
    assert lib.brush_fwd_workspace_size(1 << 20, 1920, 1080, 3, 8388480, C.byref(n)) == 0 and n.value > 0
    assert lib.brush_fwd_workspace_size(10, 32, 32, 5, 100, C.byref(n)) == -1  # sh_degree > 4
    assert lib.brush_bwd_workspace_size(1 << 20, 1920, 1080, 3, C.byref(n)) == 0 and n.value >= (1 << 20) * 36
    assert lib.brush_radix_argsort_workspace_size(1000, C.byref(n)) == 0 and n.value >= 8000
    assert lib.brush_inclusive_scan_workspace_size(1000, C.byref(n)) == 0 and n.value > 0
    # bits > 32 is rejected before any device work (brush-sort/src/lib.rs:38-39)
    assert lib.brush_radix_argsort_u32(None, None, None, None, None, 16, 33, None, 0, None) == -1
    assert lib.brush_radix_argsort_u32(None, None, None, None, None, 16, 32, None, 0, None) == -1  # null ptrs
    assert lib.brush_render_forward(None, None, None, None, None, None, 0, 0, None, None, None, 0, None) == -1
    assert lib.brush_status_string(-2) == b"workspace too small"
    # render.rs:204-206
    assert lib.brush_default_max_intersects(1 << 20, 1920, 1080) == 128 * 65535
    assert lib.brush_default_max_intersects(10, 32, 32) == 40
    assert _lib.BrushUniforms and C.sizeof(_lib.BrushUniforms) == 28 * 4


def test_camera_matches_reference_test_setup():
    """camera.rs:28-58 and the uniform packing of render.rs:102-116 vs the oracle's restatement."""
    import brush_amd
    from brush_amd.render import pack_uniforms
    from oracle import oracle as O

    w, h = 123, 82
    focal = brush_amd.fov_to_focal(math.pi * 0.5, w)
    assert abs(focal - 61.5) < 1e-12
    cam = brush_amd.Camera([0.3, -0.2, -8.0], [0.1, 0.2, 0.3, math.sqrt(1 - 0.14)], brush_amd.focal_to_fov(focal, w),
                           brush_amd.focal_to_fov(focal, h), (0.5, 0.5))
    u = pack_uniforms(cam, (w, h), 3, 10)
    o = O.make_uniforms(cam.position, cam.rotation, cam.fov_x, cam.fov_y, cam.center_uv, (w, h), 3)
    assert np.allclose(np.array(u.viewmat[:]), o["viewmat"], atol=1e-6)
    assert np.allclose(np.array(u.focal[:]), o["focal"]) and np.allclose(np.array(u.pixel_center[:]), o["pixel_center"])
    assert list(u.tile_bounds[:]) == [8, 6] and list(u.img_size[:]) == [w, h]
    # world_to_local really inverts local_to_world
    assert np.allclose(cam.world_to_local().astype(np.float64) @ cam.local_to_world(), np.eye(4), atol=1e-6)


def test_no_cpu_fallback():
    """The op refuses CPU tensors instead of silently computing elsewhere."""
    import torch

    import brush_amd

    cam = brush_amd.Camera([0, 0, -8], [0, 0, 0, 1], 1.0, 1.0)
    z = torch.zeros
    with pytest.raises(AssertionError, match="no CPU path"):
        brush_amd.render_splats(cam, (32, 32), z((4, 3)), None, z((4, 3)), z((4, 4)), z((4, 1, 3)), z((4,)))
    with pytest.raises(AssertionError):
        brush_amd.prefix_sum(torch.zeros(4, dtype=torch.int32))


def test_compositing_kernels_static_lds_and_no_spills(lib):
    """The launcher pads the compositing backward's occupancy with dynamic LDS beside the kernel's static LDS, which
    rasterize_bwd.hip derives from the kernel's own array types (bwd_static_lds, pinned there by static_asserts to the
    same literals): the descriptors of the built library must report exactly those bytes, for every instantiation, and
    neither compositing kernel may spill or use scratch."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("kernel_diff", os.path.join(ROOT, "tools", "kernel_diff.py"))
    kd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kd)
    from brush_amd import _lib

    assert lib is not None
    res = kd.resources(_lib.LIB_PATH, r"k_rasterize_(backward_)?quad")
    # (deterministic, depth) -> bytes per workgroup of 4 waves; the forward: 4 x 64 records of 48 bytes
    want_bwd = {(False, False): 39616, (False, True): 43904, (True, False): 23552, (True, True): 24576}
    seen_bwd, seen_fwd = [], 0
    for name, r in res.items():
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, name
        m = re.search(r"k_rasterize_backward_quadILj(\d)ELb([01])ELj4EJ(.*?)EEEv", name)
        if m:
            key = (int(m.group(1)), m.group(2) == "1", "DepthGrad" in m.group(3))
            assert r["group_segment_fixed_size"] == want_bwd[key[1:]], name
            seen_bwd.append(key)
        else:
            assert "k_rasterize_quadILb" in name, name
            assert r["group_segment_fixed_size"] == 12288, name
            seen_fwd += 1
    nq_det = [(1, False), (2, False), (4, False), (4, True)]
    assert sorted(seen_bwd) == sorted((nq, det, depth) for nq, det in nq_det for depth in (False, True))
    assert seen_fwd == 3


def test_per_splat_forward_kernels_static_lds_and_spills(lib):
    """The cull / compaction kernels (project.hip) and the two tile passes (tile_count.hip, tile_emit.hip): the static
    LDS of every kernel, which for the two walk kernels is one LateRing of 4608 bytes per wave (tile_walk.hpp pins the
    struct's size), every instantiation present, and no spills or scratch anywhere except the two deferred-SH degree-3
    cull kernels, which are held to exactly the 6 VGPRs / 28 bytes they spill today (recorded, unmeasured)."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("kernel_diff", os.path.join(ROOT, "tools", "kernel_diff.py"))
    kd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kd)
    from brush_amd import _lib

    assert lib is not None
    res = kd.resources(_lib.LIB_PATH, r"k_project_cull|k_cull_scan|k_compact|k_project_visible|k_walk_count|"
                                      r"k_map_intersects|k_tile_bin_edges")
    want_lds = {"k_project_cull": 4112, "k_project_visible": 4 * 4608 + 20, "k_walk_count": 4 * 4608,
                "k_map_intersects": 0, "k_tile_bin_edges": 0, "k_cull_scan": 68}
    k_aa = 8  # internal.hpp: kAaMode, beside the SH degree in the cull kernel's first template argument
    seen_cull, seen_compact, seen_other = [], [], []
    for name, r in res.items():
        m = re.search(r"\d+(k_[a-z_]+?)(?:ILi(\d+)ELb([01])EEE|ILb([01])EEE|E)", name)
        assert m, name
        kernel = m.group(1)
        spills = (r["vgpr_spill_count"], r["sgpr_spill_count"], r["private_segment_fixed_size"])
        if kernel == "k_project_cull":
            dm, lazy = int(m.group(2)), m.group(3) == "1"
            assert spills == ((6, 0, 28) if lazy and dm & 7 == 3 else (0, 0, 0)), name
            seen_cull.append((dm, lazy))
        else:
            assert spills == (0, 0, 0), name
            if kernel == "k_compact":
                assert r["group_segment_fixed_size"] == (80 if m.group(4) == "1" else 64), name
                seen_compact.append(m.group(4) == "1")
                continue
            seen_other.append(kernel)
        assert r["group_segment_fixed_size"] == want_lds[kernel], name
    assert sorted(seen_cull) == sorted([(d | aa, False) for d in range(5) for aa in (0, k_aa)] +
                                       [(d | aa, True) for d in (1, 3) for aa in (0, k_aa)])
    assert sorted(seen_compact) == [False, True]
    assert sorted(seen_other) == sorted(set(want_lds) - {"k_project_cull"})


def test_fixed_sum_kernels_static_lds_and_spills(lib):
    """The kernels that reduce through fixed_sum.hpp (pose gradient, exposure, depth loss, eval finalize): the static
    LDS of every instantiation is the staging of its wave sums and nothing else (4 waves x 12 doubles = 384 bytes;
    4 doubles + 4 uint32 = 48; 4 x 2 doubles = 64), every instantiation is present, and none spills or uses scratch."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("kernel_diff", os.path.join(ROOT, "tools", "kernel_diff.py"))
    kd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kd)
    from brush_amd import _lib

    assert lib is not None
    res = kd.resources(_lib.LIB_PATH, r"k_view_grad|k_exposure_|k_depth_loss|k_eval_finalize")
    flags, modes_types = ("Lb0E", "Lb1E"), tuple(f"Lj{m}E{t}" for m in (0, 1) for t in "ft")  # t: uint16_t
    want = {("k_view_grad", f): 384 for f in flags}
    want.update({("k_exposure_finalize", f): 384 for f in flags})
    want.update({("k_depth_loss", mt): 48 for mt in modes_types})
    want.update({("k_view_grad_finalize", None): 384, ("k_exposure_backward", None): 384,
                 ("k_exposure_forward", None): 0, ("k_depth_loss_finalize", None): 64, ("k_eval_finalize", None): 64})
    seen = []
    for name, r in res.items():
        m = re.search(r"N_1\d+(k_[a-z_]+)(?:I((?:L[bj]\d+E)[ft]?)EEv|E)", name)
        assert m, name
        key = (m.group(1), m.group(2))
        assert key in want, name
        assert (r["vgpr_spill_count"], r["sgpr_spill_count"], r["private_segment_fixed_size"]) == (0, 0, 0), name
        assert r["group_segment_fixed_size"] == want[key], name
        seen.append(key)
    assert sorted(seen, key=str) == sorted(want, key=str)


def test_sort_kernels_static_lds_and_spills(lib):
    """The kernels of the three sorters (radix_sort.hip, depth_sort.hip, tile_sort.hip): exactly these ten, each in one
    translation unit, with the static LDS of its own arrays (the scatter kernels and the depth finish take theirs as
    dynamic LDS: 0 here, or the 1024 bytes of the BUCKET scatter's splitters), and no spills or scratch: the two plain
    scatter kernels sit at 128 and 124 VGPRs, where one more live value spills."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("kernel_diff", os.path.join(ROOT, "tools", "kernel_diff.py"))
    kd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kd)
    from brush_amd import _lib

    assert lib is not None
    res = kd.resources(_lib.LIB_PATH, r"k_sort_|k_tile_bucket")
    want = {("k_sort_copy", None): 0, ("k_sort_scan", None): 20,
            ("k_sort_upsweep", "Lb0ELb0E"): 16384, ("k_sort_upsweep", "Lb1ELb0E"): 16384,
            ("k_sort_upsweep", "Lb1ELb1E"): 25600,
            ("k_sort_downsweep", "Lb1ELb0E"): 0, ("k_sort_downsweep", "Lb1ELb1E"): 1024,
            ("k_sort_downsweep_big", None): 0, ("k_sort_bucket_finish", None): 0,
            ("k_tile_bucket_finish", None): 16416}
    seen = []
    for name, r in res.items():
        m = re.search(r"N_1\d+(k_[a-z_]+?)(?:I((?:Lb[01]E){2})EEv|E)P", name)
        assert m, name
        key = (m.group(1), m.group(2))
        assert key in want, name
        assert (r["vgpr_spill_count"], r["sgpr_spill_count"], r["private_segment_fixed_size"]) == (0, 0, 0), name
        assert r["group_segment_fixed_size"] == want[key], name
        seen.append(key)
    assert sorted(seen, key=str) == sorted(want, key=str)


def test_product_and_bench_do_not_import_the_oracle():
    """The oracle is test infrastructure: importing the package, or bench.py up to its timed path
    (synthetic inputs included), must not load it; only bench.py's cpu_baseline leg and the tests do."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys, importlib.util; sys.argv=['bench.py']; import brush_amd; "
            "spec=importlib.util.spec_from_file_location('b','bench.py'); m=importlib.util.module_from_spec(spec); "
            "spec.loader.exec_module(m); m.synthetic_cloud(8, 1); "
            "print(sorted(k for k in sys.modules if k.split('.')[0] == 'oracle'))")
    out = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.strip().splitlines()[-1] == "[]"
    for dirpath, _, files in os.walk(os.path.join(root, "brush_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src, f
                assert not re.search(r"^\s*(from|import)\s+tests\b", src, flags=re.M), f
    # the bench and the tools do not depend on the test package either
    for f in ["bench.py"] + [os.path.join("tools", t) for t in os.listdir(os.path.join(root, "tools")) if t.endswith(".py")]:
        assert not re.search(r"^\s*(from|import)\s+tests\b", open(os.path.join(root, f)).read(), flags=re.M), f


def test_bench_dump_outputs_are_float_seeded_and_bounded(tmp_path):
    """bench.py --dump-outputs: float32/float64 files only, the same seeded sample of gradient rows and pixels on every
    run, the sampled rows read from the right segments of the gradient block, and under 64 MB at the headline image size
    and beyond it."""
    import importlib.util

    import torch

    from brush_amd import render as R

    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)

    class Aux:
        overflow = torch.zeros(1, dtype=torch.int32)

        def read_num_visible(self):
            return 7

        def read_num_intersections(self):
            return 11

    n, ncoef = 100_000, 16
    layout, total = R.grad_block_layout(n, ncoef)
    block = torch.rand(total, generator=torch.Generator().manual_seed(0))
    for w, h in ((1920, 1080), (2100, 1100)):
        out = torch.rand((h, w, 4), generator=torch.Generator().manual_seed(1))
        a = B.collect_outputs(out, Aux(), block, n, ncoef, with_xy=True)
        again = B.collect_outputs(out, Aux(), block, n, ncoef, with_xy=True)
        d = tmp_path / f"{w}x{h}"
        B.write_outputs(str(d), a)
        files = sorted(os.listdir(d))
        assert files == sorted(f"{k}.npy" for k in a)
        assert sum(os.path.getsize(d / f) for f in files) < 64e6
        for k, v in a.items():
            assert v.dtype in (np.float32, np.float64), k
            assert np.array_equal(v, again[k]), k
            assert np.array_equal(np.load(d / f"{k}.npy"), v), k
        rows = a["grad_index"].astype(np.int64)
        assert len(rows) == B.DUMP_GRAD_ROWS and np.all(np.diff(rows) > 0)
        for name, shape in (("v_means", (n, 3)), ("v_opac", (n,)), ("v_sh", (n, ncoef, 3)), ("v_xy", (n, 2))):
            off, sz = layout[name]
            assert np.array_equal(a[name], block[off:off + sz].view(shape).numpy()[rows]), name
        if w * h <= B.DUMP_MAX_PIXELS:
            assert "image_index" not in a and np.array_equal(a["image"], out.numpy())
        else:
            px = a["image_index"].astype(np.int64)
            assert np.array_equal(a["image"], out.reshape(-1, 4).numpy()[px])
        assert a["counts"].tolist() == [7.0, 11.0, 0.0]
