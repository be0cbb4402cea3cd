"""The baked traversal with its divisions taken from the ray's refined reciprocals (generate_baked_scene, pine_specialize.h;
ray_ordinary / make_oct / local_direction_lean, pine_device.h) against the generic nested traversal, ray by
ray, on rays aimed at what the change rests on: the ends of the ray window, zero and tiny numerators, tiny local directions.
CPU: the generated text."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

from test_obb_slabs import _box_records, _room, _source, _three_box_room, _unit

FLT_MAX = np.float32(3.4028234663852886e38)
SPAWN_TMAX = FLT_MAX * (np.float32(1.0) - np.float32(1e-3))
RAY_LO, RAY_HI = np.float32(2.0 ** -40), np.float32(2.0 ** 40)  # kRayLo, kRayHi (pine_math.h)
DIV_LO = np.float32(2.0 ** -42)                                 # kDivLo
_dn, _up = (lambda x: np.nextafter(np.float32(x), np.float32(-np.inf))), (lambda x: np.nextafter(np.float32(x), np.float32(np.inf)))
TINY_D = np.float32([RAY_LO, _up(RAY_LO), _dn(RAY_LO), RAY_LO / 2, RAY_LO * 2, DIV_LO, 2.0 ** -60, 0.0, 1e-40, 1.1754944e-38, 1e-6])
TINY_D = np.concatenate([TINY_D, -TINY_D])
# cbox (scenes.cbox): the planes of its six Rects as (axis, value) -- floor, ceiling, two side walls, back wall, lamp
CBOX_PLANES = [(1, 0.0), (1, 2.0), (0, -1.0), (0, 1.0), (2, 2.0), (1, 1.9)]


def _ordinary(rays):
    d, o = np.abs(rays[:, 3:6]), np.abs(rays[:, 0:3])
    return (d >= RAY_LO).all(axis=1) & (d <= RAY_HI).all(axis=1) & (o <= RAY_HI).all(axis=1)


def _pack(o, d, rng, short=0.3):
    n = len(o)
    tmin = np.where(rng.random(n) < 0.8, 0.0, rng.uniform(0, 0.3, n))
    tmax = np.where(rng.random(n) < short, rng.uniform(0, 3, n), SPAWN_TMAX)
    return np.concatenate([o, d, tmin[:, None], tmax[:, None]], axis=1).astype(np.float32)


def _tiny_directions(rng, n, lo, hi):
    """Origins in the room, directions with one or two components from TINY_D (the window's floor +-1 ulp, below it, the
    division's floor, zero of either sign, denormal) and the rest a unit vector."""
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    axes = np.argsort(rng.random((n, 3)), axis=1) < rng.integers(1, 3, (n, 1))
    d = _unit(np.where(axes, 0.0, rng.normal(size=(n, 3))).astype(np.float32))
    return _pack(o, np.where(axes, rng.choice(TINY_D, (n, 3)), d).astype(np.float32), rng)


def _on_planes(rng, n, planes, lo, hi):
    """Origins exactly on a Rect's plane, and 1, 2, 3 ulps and 2^-42, 2^-41, 2^-30 to either side of it (zero and tiny
    numerators); directions anywhere."""
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    which = rng.integers(0, len(planes), n)
    axis = np.array([planes[k][0] for k in which])
    value = np.float32([planes[k][1] for k in which])
    steps = rng.integers(-3, 4, n)
    moved = value.copy()
    for _ in range(3):
        moved = np.where(steps > 0, _up(moved), np.where(steps < 0, _dn(moved), moved)).astype(np.float32)
        steps = steps - np.sign(steps)
    absolute = rng.choice(np.float32([0, 2.0 ** -42, -2.0 ** -42, 2.0 ** -43, 2.0 ** -41, -2.0 ** -41, 2.0 ** -30, -2.0 ** -30, 1e-40, -0.0]), n)
    moved = np.where(rng.random(n) < 0.5, moved, (value + absolute).astype(np.float32))
    o[np.arange(n), axis] = moved
    d = _unit(rng.normal(size=(n, 3)))
    return _pack(o, d, rng)


def _huge_origins(rng, n, lo, hi):
    """Origins with a component at, just inside and beyond the window's ceiling, looking back at the room."""
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    big = np.float32([RAY_HI, _dn(RAY_HI), _up(RAY_HI), RAY_HI * 2, RAY_HI * 4, 1e30, 1e6])
    big = np.concatenate([big, -big])
    k = rng.integers(0, 3, n)
    o[np.arange(n), k] = rng.choice(big, n)
    target = rng.uniform(lo, hi, (n, 3))
    d = _unit(target - o.astype(np.float64))
    d = np.where(rng.random((n, 1)) < 0.5, d, _unit(rng.normal(size=(n, 3))))
    return _pack(o, d.astype(np.float32), rng, short=0.0)


def _along_box_axes(rng, rec, n):
    """Rays along a box's own axes, taken to world space through its matrix (columns at 6, 9, 12, translation at 15): the
    local direction M^-1 d has one component near the length and two that are rounding residue, zero, or set from TINY_D."""
    lo, hi = rec[0:3].astype(np.float64), rec[3:6].astype(np.float64)
    M = rec[6:15].reshape(3, 3).T.astype(np.float64)
    t = rec[15:18].astype(np.float64)
    k = rng.integers(0, 3, n)
    sign = rng.choice([-1.0, 1.0], n)
    dl = np.zeros((n, 3))
    dl[np.arange(n), k] = sign
    others = rng.choice(np.concatenate([TINY_D.astype(np.float64), [0.0, 0.0, 1e-9, -1e-9, 1e-7]]), (n, 3))
    others[np.arange(n), k] = 0.0
    dl = dl + others
    ol = lo + rng.uniform(-0.1, 1.1, (n, 3)) * (hi - lo)
    # on a face plane of the box for a part of the rays, outside the box along the axis for most
    ol[np.arange(n), k] = np.where(rng.random(n) < 0.8, np.where(sign > 0, lo[k] - rng.uniform(0.1, 2, n) * (hi - lo)[k], hi[k] + rng.uniform(0.1, 2, n) * (hi - lo)[k]),
                                   np.where(rng.random(n) < 0.5, lo[k], hi[k]))
    ow = ol @ M.T + t
    dw = dl @ M.T
    return _pack(ow.astype(np.float32), _unit(dw), rng)


def _compare(sc, rays):
    import pine_amd as pa
    from pine_amd import _lib
    rays = np.ascontiguousarray(rays, dtype=np.float32)
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
    assert bad.size == 0, (len(bad), bad[:5], rays[bad[:5]], [r.view(np.uint32) for r in rays[bad[:5]]], want[bad[:5]], baked[bad[:5]])
    return want


@pytest.mark.gpu
def test_cbox_rays_at_the_ends_of_the_window():
    from pine_amd import scenes
    sc = scenes.cbox((16, 16), "readme")
    assert _source(sc).count("pdiv_short(num, denom, ") == 6
    recs = _box_records(sc, (5, 6))
    rng = np.random.default_rng(9091)
    lo, hi = [-1, 0, 0], [1, 2, 2]
    sets = {"tiny directions": _tiny_directions(rng, 30000, lo, hi), "on the planes": _on_planes(rng, 36000, CBOX_PLANES, lo, hi),
            "huge origins": _huge_origins(rng, 12000, lo, hi),
            "box axes": np.concatenate([_along_box_axes(rng, rec, 11000) for rec in recs])}
    rays = np.concatenate(list(sets.values()))
    assert 90000 <= len(rays) <= 110000
    want = _compare(sc, rays)
    at = 0
    for name, q in sets.items():
        w, ordinary = want[at:at + len(q)], _ordinary(q)
        at += len(q)
        print(f"{name}: {len(q)} rays, {int(w[:, 0].sum())} hits, {int(w[:, 3].sum())} occluded, {int(ordinary.sum())} ordinary")
        # (a ray from 2^40 away misses the room by its own rounding; the other sets must meet what they are aimed at)
        assert name == "huge origins" or 0.05 < w[:, 0].mean(), (name, w[:, 0].mean())
    ordinary = _ordinary(rays)
    assert 0.2 < ordinary.mean() < 0.9, ordinary.mean()  # (the short forms and the fallback are both exercised)
    on_box = (want[:, 0] == 1) & ((want[:, 1] & 0xffff) >= 5) & ((want[:, 1] & 0xffff) <= 6)
    assert on_box.sum() > 5000 and 0.02 < want[:, 3].mean() < 0.99


@pytest.mark.gpu
def test_three_box_room_rays_at_the_ends_of_the_window():
    """No camera involved: the room tests/test_obb_slabs.py builds -- boxes rotated about two axes and scaled unevenly."""
    sc = _three_box_room()
    text = _source(sc)
    assert text.count("pdiv_short(num, denom, ") == 6 and text.count("obb_intersect<true>(") == 3
    recs = _box_records(sc, range(5, 8))
    rng = np.random.default_rng(9092)
    lo, hi = [-1, 0, 0], [1, 2, 2]
    planes = [(1, 0.0), (1, 2.0), (0, -1.0), (0, 1.0), (2, 2.0), (1, 1.9)]
    rays = np.concatenate([_tiny_directions(rng, 10000, lo, hi), _on_planes(rng, 10000, planes, lo, hi), _huge_origins(rng, 4000, lo, hi)] +
                          [_along_box_axes(rng, rec, 8000) for rec in recs])
    want = _compare(sc, rays)
    ordinary = _ordinary(rays)
    assert 0.1 < ordinary.mean() < 0.9
    on_box = (want[:, 0] == 1) & ((want[:, 1] & 0xffff) >= 5) & ((want[:, 1] & 0xffff) <= 7)
    assert on_box.sum() > 3000 and 0.02 < want[:, 3].mean() < 0.99, (on_box.sum(), want[:, 3].mean())


# ---- the generated text (no GPU) -----------------------------------------------------------------------------------
def test_generated_text_divides_by_the_rays_reciprocals(tmp_path, monkeypatch):
    import pine_amd as pa
    from pine_amd import _lib, scenes
    text = _source(scenes.cbox((640, 640), "committed"))
    # the flag is made once, where make_oct is called, and every one of cbox's six Rects takes its quotient from oct.dir_inv
    assert text.count("const bool ordinary = ray_ordinary(ray);") == 1 and text.count("make_oct(ray, ordinary)") == 1
    sites = [ln for ln in text.splitlines() if "pdiv_short(num, denom, " in ln]
    assert len(sites) == 6 and all("oct.dir_inv." in ln for ln in sites)
    assert sorted(ln.split("oct.dir_inv.")[1][0] for ln in sites) == ["x", "x", "y", "y", "y", "z"]
    assert text.count("if (__builtin_expect(!(ordinary & (pabs(num) >= kDivLo)), 0)) t = num / denom;") == 6
    assert "const float t = num / denom;" not in text
    # the sign of the reciprocal follows the sign of the normal component: denom = -ray.d.k goes with -oct.dir_inv.k
    for ln in text.splitlines():
        if ln.strip().startswith("{ const float denom = "):
            negated = "(-ray.d." in ln
            site = text.splitlines()[text.splitlines().index(ln) + 4]
            assert ("(-oct.dir_inv." in site) == negated, (ln, site)
    # a Rect whose normal component is not +-1 (state-level call: the members as given) keeps its plain division, and so does
    # one whose plane lies beyond the ray window's ceiling; an inverted box keeps the generic call
    m = pa.translate([0.0, 0.5, 1.0]) * pa.rotate_y(0.4) * pa.scale([0.5, 0.5, 0.5])
    sc = _room([([0, 0, 0], [1, -1, 1], m), ([0, 0, 0], [1, 1, 1], m)])
    f3 = C.c_float * 3
    for pos, normal in (([0.0, 1.0, 1.5], [0.0, 0.0, 0.5]), ([0.0, 1.0, 3e12], [0.0, 0.0, 1.0])):
        _lib.check(_lib.lib.pine_gpu_scene_add_rect_state(sc._h, f3(*pos), f3(0.5, 0, 0), f3(0, 0.5, 0), f3(*normal), 0.5, 0.5, f3(2, 0, 0), f3(0, 2, 0), 0), "Rect state")
    text = _source(sc)
    assert text.count("pdiv_short(num, denom, ") == 6 and text.count("const float t = num / denom;") == 2
    assert "const float denom = (ray.d.z * 0x1.000000p-1f);" in text
    assert text.count("shape_hit<F>(2,") == 1 and text.count("shape_intersect<F>(2,") == 1 and text.count("obb_hit<true>(") == 1
    # the text compiles for gfx950 (cbox; the off switch too)
    if os.path.exists("/opt/rocm/bin/hipcc") or shutil.which("hipcc"):
        monkeypatch.setenv("PINE_GPU_CACHE_DIR", str(tmp_path))
        out = C.create_string_buffer(1024)
        sc = scenes.cbox((64, 64), "committed")
        assert _lib.lib.pine_gpu_test_specialize_compile(sc._h, 258, 1536, b"gfx950", out, 1024) == 0, _lib.last_error()[-1500:]
        assert os.path.getsize(out.value.decode()) > 10000
        monkeypatch.setenv("PINE_GPU_SPECIALIZE_EXTRA", "-DPINE_NO_SHORT_DIV")
        assert _lib.lib.pine_gpu_test_specialize_compile(sc._h, 258, 1536, b"gfx950", out, 1024) == 0, _lib.last_error()[-1500:]
