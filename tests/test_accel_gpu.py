"""GPU (-m gpu): Accel's batched ray queries (include/pine_gpu.h pine_gpu_accel_*) against the real reference -- the traversal
fixtures that predate them (`pine_ref bvh`), the reference's guide images, and the records its own Accel::intersect / Accel::hit
gave for 1000 rays per scene in both orders (tools/make_golden_accel.py).  Every comparison is bit for bit: the cap on
mismatching rays is zero."""
import ctypes as C
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

import denoise_scenes
from accel_scenes import ORDERS, SEEDS, accel_scene, load_fixture, records_as_words
from conftest import GOLDEN, ROOT
from test_bvh_fixtures import SCENES as BVH_SCENES, _parse_trav, _scene as bvh_scene

pytestmark = pytest.mark.gpu
ORDER_NAME = {"bvh": "pine", "embree": "embree"}


def _same_records(got, want, what):
    got, want = records_as_words(got), records_as_words(want)
    assert got.shape == want.shape
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {len(want)} rays differ; first ray {bad[0]}: {got[bad[0]].tolist()} vs {want[bad[0]].tolist()}"


@pytest.mark.parametrize("name", BVH_SCENES)
def test_answers_equal_the_committed_traversal_fixtures(name):
    """The rays of tests/golden/bvh_*.npz: intersect's hit, geometry, triangle (on mesh hits) and t bits are the closest-hit
    words `pine_ref bvh` wrote, hit is its any-hit word."""
    import pine_amd as pa
    z = np.load(os.path.join(GOLDEN, f"bvh_{name}.npz"))
    sc = bvh_scene(name)
    assert sc.describe() == str(z["pscene"])
    rays = np.ascontiguousarray(z["rays"])
    ref = _parse_trav(z["trav"], len(rays))
    with pa.Accel(sc) as accel:
        it, occ = accel.intersect(rays), accel.hit(rays)
    bad = []
    t_bits = np.ascontiguousarray(it["t"]).view(np.uint32)
    for r, (_, (hit, geom, tri, tbits), _, any_hit) in enumerate(ref):
        ok = (it["geometry"][r] >= 0) == bool(hit) and int(t_bits[r]) == tbits and bool(occ[r]) == bool(any_hit)
        if hit:
            ok = ok and int(it["geometry"][r]) == geom and (it["triangle"][r] < 0 or int(it["triangle"][r]) == tri)
        if not ok:
            bad.append(r)
    assert not bad, f"{len(bad)} of {len(ref)} rays differ, first {bad[:5]}"
    if name in ("sss_mesh", "one_triangle"):
        assert (it["triangle"] >= 0).any()


@pytest.mark.parametrize("name", list(denoise_scenes.DENOISE_FILMS) + list(denoise_scenes.GUIDES_ONLY))
def test_normals_of_camera_rays_are_the_references_guide_image(name):
    """intersect(camera_rays()).n is DenoiseIntegrator's normal image (denoiser.cpp:13-23), bit for bit, zeros on a miss: films of
    1x1, 8x1, 45x37, 48x48 and 64x64 -- less than a wave, a ragged last block, several blocks."""
    import pine_amd as pa
    f = denoise_scenes.load(name)
    sc = denoise_scenes.denoise_scene(name)
    assert sc.describe() == f["pscene"]
    h, w = f["normal"].shape[:2]
    with pa.Accel(sc) as accel:
        assert accel.film_size == (w, h)
        rays = accel.camera_rays()
        assert rays.shape == (w * h, 8) and (rays[:, 6] == 0).all() and (rays[:, 7] == np.finfo(np.float32).max).all()
        it = accel.intersect(rays)
    want = np.ascontiguousarray(f["normal"]).reshape(w * h, 3)
    bad = (np.ascontiguousarray(it["n"]).view(np.uint32) != want.view(np.uint32)).any(axis=1)
    assert not bad.any(), f"{int(bad.sum())} of {w * h} pixels differ, first {np.nonzero(bad)[0][:5].tolist()}"
    miss = it["geometry"] < 0
    assert np.array_equal(miss, ~(want != 0).any(axis=1)) and (np.ascontiguousarray(it["p"])[miss] == 0).all()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", list(SEEDS))
def test_records_equal_the_references(name, order):
    """All 12 words of intersect and the byte of hit, for the 1000 rays of each new fixture, under Accel(BVH()) and under
    Accel(EmbreeAccel()): zero mismatching rays."""
    import pine_amd as pa
    fx = load_fixture(name, order)
    sc = accel_scene(name)
    assert sc.describe() == fx["pscene"]
    with pa.Accel(sc, order=ORDER_NAME[order]) as accel:
        it, occ = accel.intersect(fx["rays"]), accel.hit(fx["rays"])
    _same_records(it, fx["records"], f"{name}, {order}")
    bad = np.nonzero(occ.view(np.uint8) != fx["occluded"])[0]
    assert bad.size == 0, f"{name}, {order}: any-hit differs for {bad.size} rays, first {bad[:5].tolist()}"


@pytest.fixture(scope="module")
def mesh_case():
    """One accel on the mesh-with-attributes scene (global-memory variant, several BVH levels) with its 1000 rays and answers."""
    import pine_amd as pa
    fx = load_fixture("mesh_attrs", "bvh")
    accel = pa.Accel(accel_scene("mesh_attrs"))
    yield accel, fx["rays"], records_as_words(accel.intersect(fx["rays"])).copy(), accel.hit(fx["rays"]).copy()
    accel.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_a_slice_of_the_rays_gives_the_slice_of_the_answers(mesh_case, n):
    """rays[a:b] answers as rows a:b of the whole batch -- batches below a wave, at and around a wave and a 256-lane block, three
    blocks with a ragged last one (n = 600 inside the 1000) --, and nothing behind the last record of a larger output is written."""
    import torch
    accel, rays, whole, occ = mesh_case
    for a in (0, 7) if n < 1000 else (0,):
        part = np.ascontiguousarray(rays[a:a + n])
        assert np.array_equal(records_as_words(accel.intersect(part)), whole[a:a + n]), (a, n)
        assert np.array_equal(accel.hit(part), occ[a:a + n]), (a, n)
    # device buffers with room behind: n records into a buffer of n + 5 rows filled with a pattern
    from pine_amd import _lib
    count = 600 if n == 1000 else n
    d_rays = torch.from_numpy(rays).cuda()
    d_hits = torch.full((count + 5, 12), -7.25, dtype=torch.float32, device="cuda")
    d_occ = torch.full((count + 5,), 9, dtype=torch.uint8, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    first = 16  # (a row slice keeps the alignment: 16 rows of 32 bytes)
    _lib.check(_lib.lib.pine_gpu_accel_intersect_device(accel._h, C.c_void_p(d_rays[first:].data_ptr()), count, C.c_void_p(d_hits.data_ptr()), stream))
    _lib.check(_lib.lib.pine_gpu_accel_hit_device(accel._h, C.c_void_p(d_rays[first:].data_ptr()), count, C.c_void_p(d_occ.data_ptr()), stream))
    torch.cuda.synchronize()
    got = d_hits.cpu().numpy()
    assert np.array_equal(got[:count].view(np.uint32), whole[first:first + count])
    assert (got[count:] == -7.25).all()
    assert np.array_equal(d_occ.cpu().numpy()[:count], occ[first:first + count].view(np.uint8)) and (d_occ.cpu().numpy()[count:] == 9).all()


def test_zero_rays_and_bad_buffers(mesh_case):
    """n == 0 returns 0 and launches nothing; misaligned device pointers and a negative count fail before a launch; the
    wrapper raises ValueError for rays on the wrong device, of the wrong dtype, shape or layout."""
    import torch
    from pine_amd import _lib
    accel, rays, whole, occ = mesh_case
    assert len(accel.intersect(np.zeros((0, 8), np.float32))) == 0 and len(accel.hit(np.zeros((0, 8), np.float32))) == 0
    d_rays = torch.from_numpy(rays).cuda()
    d_hits = torch.full((8, 12), 3.5, dtype=torch.float32, device="cuda")
    assert _lib.lib.pine_gpu_accel_intersect_device(accel._h, C.c_void_p(d_rays.data_ptr()), 0, C.c_void_p(d_hits.data_ptr()), None) == 0
    empty = accel.intersect(d_rays[:0])
    assert tuple(empty.records.shape) == (0, 12)
    assert _lib.lib.pine_gpu_accel_intersect_device(accel._h, C.c_void_p(d_rays.data_ptr() + 4), 4, C.c_void_p(d_hits.data_ptr()), None) < 0
    assert "16-byte aligned" in _lib.last_error()
    assert _lib.lib.pine_gpu_accel_intersect_device(accel._h, C.c_void_p(d_rays.data_ptr()), 4, C.c_void_p(d_hits.data_ptr() + 8), None) < 0
    assert _lib.lib.pine_gpu_accel_intersect_device(accel._h, C.c_void_p(d_rays.data_ptr()), -1, C.c_void_p(d_hits.data_ptr()), None) < 0
    torch.cuda.synchronize()
    assert (d_hits.cpu().numpy() == 3.5).all()
    for bad in (d_rays.double(), d_rays[:, :7], d_rays.reshape(-1), d_rays[:, :4].repeat(1, 4)[:, ::2], torch.from_numpy(rays)):
        with pytest.raises(ValueError):
            accel.intersect(bad)
        with pytest.raises(ValueError):
            accel.hit(bad)


def test_host_arrays_device_pointers_and_tensors_give_the_same_bytes(mesh_case):
    """The three input forms; and two torch streams querying the one accel at once answer as one stream does."""
    import torch
    from pine_amd import _lib
    accel, rays, whole, occ = mesh_case
    d_rays = torch.from_numpy(rays).cuda()
    it = accel.intersect(d_rays)
    d_occ = accel.hit(d_rays)
    assert it.records.is_cuda and it.records.dtype == torch.float32 and tuple(it.records.shape) == (len(rays), 12)
    assert d_occ.dtype == torch.uint8 and it.geometry.dtype == torch.int32 and it.geometry.data_ptr() == it.records.data_ptr() + 4
    assert np.array_equal(it.records.cpu().numpy().view(np.uint32), whole) and np.array_equal(d_occ.cpu().numpy(), occ.view(np.uint8))
    host = accel.intersect(rays)
    assert np.array_equal(it.t.cpu().numpy(), host["t"]) and np.array_equal(it.geometry.cpu().numpy(), host["geometry"])
    assert np.array_equal(it.triangle.cpu().numpy(), host["triangle"]) and np.array_equal(it.material.cpu().numpy(), host["material"])
    assert np.array_equal(it.p.cpu().numpy(), host["p"]) and np.array_equal(it.n.cpu().numpy(), host["n"]) and np.array_equal(it.uv.cpu().numpy(), host["uv"])
    raw = torch.zeros((len(rays), 12), dtype=torch.float32, device="cuda")
    _lib.check(_lib.lib.pine_gpu_accel_intersect_device(accel._h, C.c_void_p(d_rays.data_ptr()), len(rays), C.c_void_p(raw.data_ptr()),
                                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert np.array_equal(raw.cpu().numpy().view(np.uint32), whole)
    # two streams at once, several rounds each
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    halves = [d_rays[:512].contiguous(), d_rays[512:].contiguous()]
    outs = [[], []]
    for _ in range(4):
        for k, s in enumerate(streams):
            with torch.cuda.stream(s):
                outs[k].append((accel.intersect(halves[k]).records, accel.hit(halves[k])))
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(((0, 512), (512, len(rays)))):
        for rec, oc in outs[k]:
            assert np.array_equal(rec.cpu().numpy().view(np.uint32), whole[a:b]) and np.array_equal(oc.cpu().numpy(), occ[a:b].view(np.uint8))


def test_an_accel_is_a_snapshot_of_its_scene():
    """A shape added after Accel(...) is not in it; a second accel sees it."""
    import pine_amd as pa
    from pine_amd import scenes
    sc = scenes.cbox((16, 16), "readme")
    rays = np.zeros((64, 8), np.float32)
    rays[:, 0:3] = [0, 1, -4]
    gx, gy = np.meshgrid(np.linspace(-0.2, 0.2, 8), np.linspace(-0.2, 0.2, 8))
    rays[:, 3], rays[:, 4], rays[:, 5], rays[:, 7] = gx.ravel(), gy.ravel(), 1.0, np.finfo(np.float32).max
    with pa.Accel(sc) as first:
        before = records_as_words(first.intersect(rays)).copy()
        sc.add(pa.Sphere([0, 1, -2], 0.5), "red")  # in front of everything
        assert np.array_equal(records_as_words(first.intersect(rays)), before)
        with pa.Accel(sc) as second:
            after = second.intersect(rays)
        assert np.array_equal(records_as_words(first.intersect(rays)), before)
    new = after["geometry"] == after["geometry"].max()
    assert new.sum() >= 4 and (after["t"][new] < before[new, 0].view(np.float32)).all()
    assert np.array_equal(records_as_words(after)[~new], before[~new])


def test_a_bvh_of_more_than_65536_nodes_is_answered_like_the_generic_kernel():
    """An icosphere of 327 680 triangles (the mesh of the beyond-16-bit test of tests/test_gpu_parity.py): the accel's 32-bit
    stack in LDS; its answers are those of the all-features traversal hook, for a few hundred rays."""
    import pine_amd as pa
    from pine_amd import _lib, scenes
    sc = scenes.sss((24, 24), 7, skin=pa.Glossy([0.9, 0.5, 0.3], 0.2))
    assert _lib.lib.pine_gpu_scene_build_accel(sc._h) >= 65536
    rng = np.random.default_rng(5)
    n = 300
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3] = [0, 1, -4]
    d = np.array([0.0, -0.5, 5.0]) + rng.uniform(-0.45, 0.45, (n, 3)) * [1, 1, 0]  # towards the sphere at (0, 0.5, 1)
    rays[:, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays[:, 7] = np.finfo(np.float32).max
    cap = 2
    out = np.zeros((n, 2 * cap + 5), np.uint32)
    _lib.check(_lib.lib.pine_gpu_test_traverse(sc._h, 0, rays.ctypes.data_as(_lib.c_f_p), n, 0, cap, out.ctypes.data_as(C.POINTER(C.c_uint32))))
    with pa.Accel(sc) as accel:
        assert not accel.kernel_features & (1 << 8) and not accel.kernel_features & (1 << 13)  # (neither F_LDS_SCENE nor F_LDS_TOP)
        it, occ = accel.intersect(rays), accel.hit(rays)
    hit = out[:, cap] == 1
    assert np.array_equal(it["geometry"] >= 0, hit) and np.array_equal(np.ascontiguousarray(it["t"]).view(np.uint32), out[:, cap + 3])
    assert np.array_equal(it["geometry"][hit], out[hit, cap + 1].view(np.int32))
    mesh = it["triangle"] >= 0
    assert mesh.sum() >= 50 and np.array_equal(it["triangle"][mesh], out[mesh, cap + 2].view(np.int32))
    assert np.array_equal(occ.view(np.uint8), out[:, 2 * cap + 4].astype(np.uint8))


def test_the_custom_integrator_example_writes_a_picture(tmp_path):
    """examples/custom_integrator.py at 32 x 32: a PNG whose pixels are finite and not all equal."""
    from test_abi import _decode_png_rgba8
    out = str(tmp_path / "custom.png")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "custom_integrator.py"), "32", out], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    px = _decode_png_rgba8(out)
    assert px.shape == (32, 32, 4) and np.isfinite(px.astype(np.float64)).all()
    assert len(np.unique(px[..., 0])) > 8, "a flat picture"
    import importlib.util
    spec = importlib.util.spec_from_file_location("custom_integrator", os.path.join(ROOT, "examples", "custom_integrator.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    film = mod.render(32)
    assert np.isfinite(film).all() and film[..., :3].min() >= 0 and film[..., :3].max() <= 1 and 0 < (film[..., 0] > 0).mean() < 1


@pytest.mark.parametrize("order", ORDERS)
def test_cpp_facade_agrees_with_python_on_64_rays(tmp_path, order):
    """examples/ray_queries.cpp (pine::Accel over host arrays) compiles, runs and writes the records the Python interface gives
    for the scene it describes and the rays it made."""
    import pine_amd as pa
    from pine_amd import scenes
    exe, lib_dir = str(tmp_path / "ray_queries"), os.path.join(ROOT, "pine_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", os.path.join(ROOT, "examples", "ray_queries.cpp"), "-L" + lib_dir, "-lpine_gpu",
                           "-Wl,-rpath," + lib_dir, "-o", exe])
    out, ps = str(tmp_path / "out.bin"), str(tmp_path / "out.pscene")
    r = subprocess.run([exe, order, out, ps], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    sc = scenes.cbox((64, 64), "readme")
    assert open(ps).read() == sc.describe()
    raw = np.fromfile(out, dtype=np.uint8)
    assert raw.size == 64 * (32 + 48 + 1)
    rays = raw[:64 * 32].view(np.float32).reshape(64, 8).copy()
    rec = raw[64 * 32:64 * 80].view(np.uint32).reshape(64, 12)
    occ = raw[64 * 80:]
    with pa.Accel(sc, order=ORDER_NAME[order]) as accel:
        it, mine = accel.intersect(rays), accel.hit(rays)
    _same_records(it, rec, "C++ facade")
    assert np.array_equal(mine.view(np.uint8), occ) and 0 < (it["geometry"] >= 0).sum() < 64


def test_closed_accels_leave_nothing_behind():
    """pine_gpu_test_live_device_blocks is back where it was after accels of both orders and of both kernel families were made,
    queried (host and device forms) and closed -- and after one whose creation failed half way."""
    import torch
    import pine_amd as pa
    from pine_amd import _lib

    def live():
        out = (C.c_int64 * 2)()
        _lib.check(_lib.lib.pine_gpu_test_live_device_blocks(out))
        return int(out[0])

    gc.collect()
    torch.cuda.synchronize()
    start = live()
    for name in ("cbox", "sss_mesh"):
        fx = load_fixture(name, "bvh")
        for order in ("pine", "embree"):
            accel = pa.Accel(accel_scene(name), order=order)
            assert live() > start
            accel.intersect(fx["rays"]), accel.hit(fx["rays"]), accel.camera_rays()
            accel.hit(torch.from_numpy(fx["rays"]).cuda())
            accel.close()
            accel.close()  # (twice is fine)
            with pytest.raises(pa.PineError, match="closed"):
                accel.hit(fx["rays"])
            assert live() == start, (name, order)
    os.environ["PINE_GPU_ACCEL_VARIANT"] = "0"  # (the analytic, scene-in-LDS variant cannot take a mesh: creation fails after the upload)
    try:
        with pytest.raises(pa.PineError, match="PINE_GPU_ACCEL_VARIANT"):
            pa.Accel(accel_scene("sss_mesh"))
    finally:
        del os.environ["PINE_GPU_ACCEL_VARIANT"]
    assert live() == start
