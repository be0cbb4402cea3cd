"""The slab test of baked scenes' transformed boxes (box_slabs_lean and obb_hit<true> / obb_intersect<true>,
pine_amd/csrc/pine_device.h; emitted by generate_baked_scene, pine_specialize.h) must answer what box_slabs answers for every
ray the path kernel creates: finite origin, finite direction that is not zero, tmin >= 0.
CPU: the host builds of the two routines side by side on about a million constructed rays; the generated text.
GPU: the baked traversal against the generic one ray by ray, on rays aimed at the boxes in each box's own frame; films."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

from conftest import assert_bit_equal, load_film

FLT_MAX = np.float32(3.4028234663852886e38)
SPAWN_TMAX = FLT_MAX * (np.float32(1.0) - np.float32(1e-3))  # spawn_ray's tmax for an unbounded ray
EPS = np.float32(1e-6)                                       # box_slabs' threshold of a parallel axis
TINY = np.float32([np.nextafter(EPS, np.float32(0)), EPS, np.nextafter(EPS, np.float32(1)), 1e-5])
TINY = np.concatenate([TINY, -TINY])


def _unit(d):
    n = np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)
    return (d / np.maximum(n, 1e-300)).astype(np.float32)


def _some_axes(rng, n, count):
    """Per row, `count` of the three axes chosen at random (a boolean mask)."""
    return np.argsort(rng.random((n, 3)), axis=1) < count


def _on_planes(rng, lo, hi, n, count):
    """Origins with `count` coordinates exactly on a face plane of their box (1: a face plane, 2: an edge line, 3: a corner);
    the other coordinates within or around the box, so that face and edge origins lie on the box and beside it."""
    o = (lo + rng.uniform(-0.25, 1.25, (n, 3)) * (hi - lo)).astype(np.float32)
    return np.where(_some_axes(rng, n, count), np.where(rng.random((n, 3)) < 0.5, lo, hi), o).astype(np.float32)


def _classes(rng, lo, hi, per):
    """Local-frame rays by class: {name: (origins, directions)}; lo / hi are (per, 3) arrays of boxes."""
    ext = hi - lo
    around = lambda: (lo + rng.uniform(-1.5, 2.5, (per, 3)) * ext).astype(np.float32)
    inside = lambda: (lo + rng.uniform(0.0, 1.0, (per, 3)) * ext).astype(np.float32)
    anydir = lambda: _unit(rng.normal(size=(per, 3)))
    mixed = lambda: np.where(rng.random((per, 1)) < 0.5, around(), inside())
    out = {"random": (around(), anydir()), "face": (_on_planes(rng, lo, hi, per, 1), anydir()),
           "edge": (_on_planes(rng, lo, hi, per, 2), anydir()), "corner": (_on_planes(rng, lo, hi, per, 3), anydir()),
           "inside": (inside(), anydir())}
    for name, k in (("zero1", 1), ("zero2", 2)):  # one / two components exactly zero, of either sign
        d = _unit(np.where(_some_axes(rng, per, k), np.float32(0.0), anydir()))
        out[name] = (mixed(), np.where((d == 0) & (rng.random((per, 3)) < 0.5), np.float32(-0.0), d))
    for name, k in (("tiny1", 1), ("tiny2", 2)):  # ... at +-1e-6 -+ 1 ulp (either side of the parallel threshold) and at 1e-5
        axes = _some_axes(rng, per, k)
        d = _unit(np.where(axes, np.float32(0.0), anydir()))
        out[name] = (mixed(), np.where(axes, rng.choice(TINY, (per, 3)), d).astype(np.float32))
    # along the box's diagonals, through a corner or just beside it
    sign = rng.choice(np.float32([-1, 1]), (per, 3))
    d = _unit(sign * ext)
    corner = np.where(sign > 0, lo, hi)
    o = (corner - rng.uniform(0.5, 3.0, (per, 1)).astype(np.float32) * d).astype(np.float32)
    o = np.where(rng.random((per, 1)) < 0.5, o, o + (rng.normal(size=(per, 3)) * 0.05 * ext).astype(np.float32)).astype(np.float32)
    out["diagonal"] = (o, d)
    return out


def _slabs(lo, hi, rays):
    from pine_amd import _lib
    boxes = np.ascontiguousarray(np.concatenate([lo, hi], axis=1), dtype=np.float32)
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    out = np.zeros((len(rays), 6), dtype=np.uint32)
    _lib.check(_lib.lib.pine_gpu_test_box_slabs(boxes.ctypes.data_as(_lib.c_f_p), rays.ctypes.data_as(_lib.c_f_p), len(rays),
                                                out.ctypes.data_as(C.POINTER(C.c_uint32))), "pine_gpu_test_box_slabs")
    return out


def _boxes(rng, n):
    lo = rng.uniform(-2, 1, (n, 3)).astype(np.float32)
    hi = (lo + rng.uniform(0.05, 2, (n, 3)).astype(np.float32)).astype(np.float32)
    k = n // 4
    lo[:k], hi[:k] = 0.0, 1.0                                  # the unit box every Box() of the scenes is
    flat = rng.integers(0, 3, k)
    hi[k:2 * k][np.arange(k), flat] = lo[k:2 * k][np.arange(k), flat]  # lo == hi on one axis
    return lo, hi


def test_lean_slabs_equal_box_slabs_on_constructed_rays():
    """Flag, and on a hit the bits of tmin and tmax, of box_slabs_lean against box_slabs (host builds, -ffp-contract=off as the
    device code).  Every class of rays must hold hits and misses."""
    rng = np.random.default_rng(20251)
    per = 60000
    lo, hi = _boxes(rng, per)
    total = 0
    for name, (o, d) in _classes(rng, lo, hi, per).items():
        n = len(o)
        tmin = np.where(rng.random(n) < 0.75, 0.0, rng.uniform(0, 3, n)).astype(np.float32)
        tmax = rng.choice(np.float32([FLT_MAX, SPAWN_TMAX]), n)
        rays = np.concatenate([o, d, tmin[:, None], tmax[:, None]], axis=1).astype(np.float32)
        # short rays: from the unbounded ray's own interval [t0, t1] -- ending before the box, a hair before it, on it, a hair
        # inside, half way through, and on the far side
        r = _slabs(lo, hi, rays)
        t0, t1 = r[:, 1].copy().view(np.float32), r[:, 2].copy().view(np.float32)
        sel = np.nonzero((r[:, 0] == 1) & (t1 < FLT_MAX / 4))[0]
        ends = np.stack([t0[sel] * np.float32(0.5), np.nextafter(t0[sel], np.float32(0)), t0[sel], np.nextafter(t0[sel], FLT_MAX),
                         (t0[sel] + t1[sel]) * np.float32(0.5), t1[sel]], axis=1)
        pick = rng.integers(0, ends.shape[1], len(sel))
        short = rays[sel].copy()
        short[:, 7] = ends[np.arange(len(sel)), pick]
        for what, (bl, bh, q) in {name: (lo, hi, rays), name + " (short)": (lo[sel], hi[sel], short)}.items():
            r = _slabs(bl, bh, q)
            gen, lean = r[:, :3], r[:, 3:]
            bad = np.nonzero(gen[:, 0] != lean[:, 0])[0]
            assert bad.size == 0, (what, "flag", q[bad[:3]], bl[bad[:3]], bh[bad[:3]], r[bad[:3]])
            hit = gen[:, 0] == 1
            bad = np.nonzero(hit & ((gen[:, 1] != lean[:, 1]) | (gen[:, 2] != lean[:, 2])))[0]
            assert bad.size == 0, (what, "bounds", q[bad[:3]], bl[bad[:3]], bh[bad[:3]], r[bad[:3]])
            assert 0 < hit.sum() < len(q), (what, int(hit.sum()), len(q))  # (hits and misses: no class degenerates)
            print(f"{what}: {len(q)} rays, {int(hit.sum())} hits")
            total += len(q)
    assert total > 900000


# ---- the generated text ---------------------------------------------------------------------------------------------
def _source(scene):
    from pine_amd import _lib
    n = _lib.lib.pine_gpu_scene_specialized_source(scene._h, None, 0)
    assert n >= 0, _lib.last_error()
    buf = C.create_string_buffer(n + 1)
    _lib.lib.pine_gpu_scene_specialized_source(scene._h, buf, n + 1)
    return buf.value.decode()


def _room(boxes):
    """Five walls and a lamp around `boxes` (lower, upper, matrix)."""
    import pine_amd as pa
    sc = pa.Scene()
    sc.add("w", pa.Diffuse([0.7, 0.7, 0.7]))
    for pos, ex, ey, flip in (([0, 0, 1], [2, 0, 0], [0, 0, 2], True), ([0, 2, 1], [2, 0, 0], [0, 0, 2], False), ([-1, 1, 1], [0, 0, 2], [0, 2, 0], True),
                              ([1, 1, 1], [0, 0, 2], [0, 2, 0], False), ([0, 1, 2], [2, 0, 0], [0, 2, 0], True)):
        sc.add(pa.Rect(pos, ex, ey, flip), "w")
    for lower, upper, m in boxes:
        sc.add(pa.Box(pa.AABB(lower, upper), m), "w")
    sc.add(pa.Rect([0.0, 1.9, 1], [0.5, 0, 0], [0, 0, 0.5]), pa.Emissive([20.0, 18.0, 15.0]))
    sc.set(pa.ThinLenCamera(pa.Film([16, 16]), [0, 1, -4], [0, 1, 0], 0.25))
    return sc


def _three_box_room():
    import pine_amd as pa
    return _room([([0, 0, 0], [1, 1, 1], pa.translate([0.1, 0.3, 0.7]) * pa.rotate_x(0.5) * pa.rotate_z(-0.3) * pa.scale([0.5, 0.2, 0.8])),
                  ([-1, -1, -1], [1, 1, 1], pa.translate([-0.5, 1.2, 1.3]) * pa.rotate_z(1.1) * pa.rotate_y(0.7) * pa.scale([0.15, 0.4, 0.25])),
                  ([0, -0.5, 0.25], [2, 0.5, 0.75], pa.translate([0.3, 1.4, 0.9]) * pa.rotate_y(-0.9) * pa.rotate_x(2.0) * pa.scale([0.2, 0.6, 0.3]))])


def test_generated_text_calls_the_lean_tests_for_ordinary_boxes(tmp_path, monkeypatch):
    import pine_amd as pa
    from pine_amd import _lib, scenes
    text = _source(scenes.cbox((64, 64), "readme"))
    assert text.count("obb_hit<true>(rec.f, ray)") == 2 and text.count("obb_intersect<true>(rec.f, ray)") == 2
    assert "shape_hit<F>(2," not in text and "shape_intersect<F>(2," not in text
    text = _source(_three_box_room())
    assert text.count("obb_hit<true>(rec.f, ray)") == 3 and "shape_hit<F>(2," not in text
    # an inverted box (lo > hi on an axis: never hit) keeps the generic call; the ordinary box beside it does not
    m = pa.translate([0.0, 0.5, 1.0]) * pa.rotate_y(0.4) * pa.scale([0.5, 0.5, 0.5])
    text = _source(_room([([0, 0, 0], [1, -1, 1], m), ([0, 0, 0], [1, 1, 1], m)]))
    assert text.count("shape_hit<F>(2,") == 1 and text.count("shape_intersect<F>(2,") == 1 and text.count("obb_hit<true>(") == 1
    # a box with a bound that is not finite is not baked at all (the record has no literal): no lean call, the generic traversal
    assert "obb_hit<true>" not in _source(_room([([0, 0, 0], [1, float("inf"), 1], m)]))
    if os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc"):
        monkeypatch.setenv("PINE_GPU_CACHE_DIR", str(tmp_path))
        out = C.create_string_buffer(1024)
        sc = scenes.cbox((64, 64), "readme")
        assert _lib.lib.pine_gpu_test_specialize_compile(sc._h, 258, 1536, b"gfx950", out, 1024) == 0, _lib.last_error()[-1500:]
        assert os.path.getsize(out.value.decode()) > 10000


# ---- GPU ------------------------------------------------------------------------------------------------------------
def _box_records(sc, geometries):
    from pine_amd import _lib
    recs = []
    for g in geometries:
        rec = (C.c_float * 32)()
        _lib.check(_lib.lib.pine_gpu_scene_shape_record(sc._h, g, rec))
        recs.append(np.frombuffer(rec, dtype=np.float32).copy())
    return recs


def _world_rays(rng, rec, per):
    """The constructed classes in the box's own frame, taken to world space with the record's matrix (columns at 6, 9, 12,
    translation at 15), plus shadow-style rays that end just before a face."""
    lo, hi = np.tile(rec[0:3], (per, 1)), np.tile(rec[3:6], (per, 1))
    M = rec[6:15].reshape(3, 3).T.astype(np.float64)  # (columns x, y, z)
    t = rec[15:18].astype(np.float64)
    rays = []
    for name, (o, d) in _classes(rng, lo, hi, per).items():
        ow = (o.astype(np.float64) @ M.T + t).astype(np.float32)
        dw = _unit(d.astype(np.float64) @ M.T)
        tmin = np.where(rng.random(per) < 0.75, 0.0, rng.uniform(0, 0.5, per)).astype(np.float32)
        tmax = np.where(rng.random(per) < 0.7, SPAWN_TMAX, rng.uniform(0, 4, per)).astype(np.float32)
        rays.append(np.concatenate([ow, dw, tmin[:, None], tmax[:, None]], axis=1))
    # shadow rays: from a point of the room to a point on a face, ending 1e-3 (spawn_ray), a few ulps or nothing before it
    face = _on_planes(rng, lo, hi, per, 1)
    face = np.clip(face, lo, hi)
    target = face.astype(np.float64) @ M.T + t
    o = rng.uniform([-1, 0, 0], [1, 2, 2], (per, 3))
    dist = np.linalg.norm(target - o, axis=1)
    short = rng.choice([1.0 - 1e-3, 1.0 - 1e-6, 1.0 - 2.0 ** -23, 1.0, 1.0 + 1e-6], per)
    rays.append(np.concatenate([o, (target - o) / dist[:, None], np.zeros((per, 1)), (dist * short)[:, None]], axis=1))
    return np.ascontiguousarray(np.concatenate(rays), dtype=np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["cbox", "three_boxes"])
def test_baked_boxes_equal_the_generic_traversal_ray_by_ray(which):
    """The scene's kernel's traversal (the lean box tests) against the generic nested traversal: hit flag, geometry word, tmax
    bits and the any-hit answer, on rays aimed at each box in its own frame."""
    import pine_amd as pa
    from pine_amd import _lib, scenes
    sc = scenes.cbox((16, 16), "readme") if which == "cbox" else _three_box_room()
    recs = _box_records(sc, range(5, 5 + (2 if which == "cbox" else 3)))  # (the walls are geometries 0-4, the boxes follow)
    assert _source(sc).count("obb_intersect<true>(") == len(recs)
    rng = np.random.default_rng(77)
    per = 19800 // (len(recs) * 11)
    rays = np.concatenate([_world_rays(rng, rec, per) for rec in recs])
    assert len(rays) <= 20000
    cap = 40
    gen = np.zeros((len(rays), 2 * cap + 5), dtype=np.uint32)
    _lib.check(_lib.lib.pine_gpu_test_traverse(sc._h, 0, rays.ctypes.data_as(_lib.c_f_p), len(rays), 0, cap, gen.ctypes.data_as(C.POINTER(C.c_uint32))))
    plan = pa.Plan(sc, 1, 1, specialize=True)
    assert plan.stats().specialized == 2
    baked = np.zeros((len(rays), 4), dtype=np.uint32)
    _lib.check(_lib.lib.pine_gpu_plan_test_traverse_baked(plan._h, rays.ctypes.data_as(_lib.c_f_p), len(rays), baked.ctypes.data_as(C.POINTER(C.c_uint32))))
    plan.close()
    want = np.stack([gen[:, cap], gen[:, cap + 1], gen[:, cap + 3], gen[:, 2 * cap + 4]], axis=1)
    bad = np.nonzero((want != baked).any(axis=1))[0]
    assert bad.size == 0, (len(bad), bad[:5], rays[bad[:5]], want[bad[:5]], baked[bad[:5]])
    # the rays do meet the boxes, and the any-hit answers differ among them
    on_box = (want[:, 0] == 1) & ((want[:, 1] & 0xffff) >= 5) & ((want[:, 1] & 0xffff) < 5 + len(recs))
    assert on_box.mean() > 0.2 and 0.05 < want[:, 3].mean() < 0.99, (on_box.mean(), want[:, 3].mean())


def _render(scene, spp, depth, **kw):
    import torch
    import pine_amd as pa
    w, h = scene.camera.film().size
    plan = pa.Plan(scene, spp, depth, **kw)
    film = torch.full((h, w, 4), -1.0, dtype=torch.float32, device="cuda")
    plan.launch(film.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    plan.check()
    st = plan.stats()
    out = film.cpu().numpy()
    plan.close()
    return out, st


@pytest.mark.gpu
def test_cbox_film_of_the_scene_kernel_equals_the_precompiled_one_and_the_reference():
    from pine_amd import scenes
    ref, ps, spp, depth = load_film("cbox_readme_64_s16_d8")
    assert (spp, depth) == (16, 8)
    sc = scenes.cbox((64, 64), "readme")
    assert sc.describe() == ps
    own, st = _render(sc, spp, depth, specialize=True)
    pre, st0 = _render(sc, spp, depth, specialize=False)
    assert st.specialized == 2 and st0.specialized == 0
    assert_bit_equal(own, pre, "the scene's kernel vs the precompiled kernel")
    assert_bit_equal(own, ref, "the scene's kernel vs the reference's film")
    assert st.vertices == st0.vertices and st.shadow_rays == st0.shadow_rays and st.vertices > 64 * 64 * 16
