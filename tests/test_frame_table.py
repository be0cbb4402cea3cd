"""The frame table: the world normal and the tangent frame of every face of a Rect, an AABB or an OBB, evaluated once
at plan creation and looked up by the path kernels instead of recomputed at every hit.

CPU: the table against the per-hit functions it replaces (host build) and against the reference's hit records.
GPU: films with the table are the golden films, bit for bit, in every kernel; $PINE_GPU_FRAME_TABLE=0 gives the same bytes; a plan
whose kernel choice the table's bytes would change has none.  (That last check creates plans, so it needs the device too.)"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, assert_bit_equal, load_film
from film_scenes import film_scene

FLAT_KINDS = {"rect": 1, "box": 6, "obb": 6}  # (the shape words of Scene.describe)


def frame_table(scene, plan=None, rays=None):
    """(entries [n, 12], generic [n, 12], base [geometries], faces [non-mesh geometries, rays] or None)."""
    from pine_amd import _lib
    cap, shapes = 4096, 1024
    entries = np.zeros((cap, 12), np.float32)
    generic = np.zeros((cap, 12), np.float32)
    base = np.full(shapes, -2, np.int32)
    faces = None
    if rays is not None:
        rays = np.ascontiguousarray(rays, np.float32)
        faces = np.full(shapes * len(rays), -2, np.int32)
    n = _lib.check(_lib.lib.pine_gpu_test_frame_table(
        scene._h, plan._h if plan is not None else None, 0 if plan is not None else -1, entries.ctypes.data_as(_lib.c_f_p),
        generic.ctypes.data_as(_lib.c_f_p), cap, base.ctypes.data_as(C.POINTER(C.c_int32)), shapes,
        rays.ctypes.data_as(_lib.c_f_p) if rays is not None else None, len(rays) if rays is not None else 0,
        faces.ctypes.data_as(C.POINTER(C.c_int32)) if faces is not None else None), "pine_gpu_test_frame_table")
    base = base[base != -2]
    if faces is not None:
        faces = faces[faces != -2].reshape(-1, len(rays))
    return entries[:n], generic[:n], base, faces


def edge_scene():
    """Flat shapes at the edges of the two functions: normals with +0 and -0 components, the tie |n.x| == |n.y| of
    coordinate_system, boxes rotated about each axis, non-uniform scale, a mirroring transform."""
    import pine_amd as pa
    s = pa.Scene()
    s.add("d", pa.Diffuse([0.8, 0.8, 0.8]))
    for flip in (False, True):
        s.add(pa.Rect([0, 0, 1], [2, 0, 0], [0, 0, 2], flip), "d")   # n = (+-0, -+1, +-0)
        s.add(pa.Rect([1, 1, 1], [0, 0, 2], [0, 2, 0], flip), "d")   # along x
        s.add(pa.Rect([0, 1, 2], [2, 0, 0], [0, 2, 0], flip), "d")   # along z
        s.add(pa.Rect([0, 1, 1], [1, -1, 0], [0, 0, 1], flip), "d")  # |n.x| == |n.y|
        s.add(pa.Rect([0, 1, 1], [1, 1, 0], [0, 0, 1], flip), "d")   # ... with opposite signs
    s.add(pa.Rect([0.3, 0.2, 0.1], [0.3, 0.1, -0.2], [0.05, 0.4, 0.1]), "d")
    s.add(pa.Box([-0.9, 0.0, 0.2], [-0.5, 0.5, 0.6]), "d")
    unit = pa.AABB([0, 0, 0], [1, 1, 1])
    for m in (pa.rotate_x(0.7), pa.rotate_y(-1.1), pa.rotate_z(2.3), pa.rotate_z(np.pi / 4),
              pa.translate([0.1, 0.2, 0.3]) * pa.rotate_x(0.3) * pa.rotate_z(-1.1) * pa.scale([0.2, 1.7, 0.6]),
              pa.scale([-1.0, 1.0, 1.0]), pa.translate([0, 1, 0]) * pa.rotate_y(0.4) * pa.scale([0.5, -2.0, 0.25]), pa.scale([1e-3, 1e3, 1.0])):
        s.add(pa.Box(unit, m), "d")
    s.add(pa.Box(pa.AABB([-0.2, 0.1, -3.0], [0.9, 0.15, 5.0]), pa.rotate_y(0.4)), "d")
    s.add(pa.Sphere([0.5, 0.3, 1.2], 0.3), "d")
    s.add(pa.Rect([0.0, 1.9, 1], [0.1, 0, 0], [0, 0, 0.1]), pa.Emissive([10.0, 10.0, 10.0]))
    s.set(pa.ThinLenCamera(pa.Film([16, 16]), [0, 1, -4], [0, 1, 0], 0.25))
    return s


def kinds_of(scene):
    return [ln.split()[1] for ln in scene.describe().splitlines() if ln.startswith("shape ")]


def _scene(which):
    from pine_amd import scenes
    return {"cbox": lambda: scenes.cbox((64, 64)), "shapes_zoo": lambda: scenes.shapes_zoo((48, 48)), "edges": edge_scene}[which]()


@pytest.mark.parametrize("which", ["cbox", "shapes_zoo", "edges"])
def test_table_equals_the_functions_it_replaces(which):
    """Every entry, bit for bit, is what the host build of shape_surface_info and coordinate_system returns at a point of that
    shape's face; every flat shape has its entries, in geometry order, and no other shape has any."""
    sc = _scene(which)
    entries, generic, base, _ = frame_table(sc)
    kinds = kinds_of(sc)
    assert len(base) == len(kinds)
    at = 0
    for g, kind in enumerate(kinds):
        faces = FLAT_KINDS.get(kind, 0)
        assert base[g] == (at if faces else -1), (g, kind)
        at += faces
    assert at == len(entries) and at > 0
    assert_bit_equal(entries, generic, f"{which}: frame table vs shape_surface_info + coordinate_system")
    if which == "cbox":
        assert len(entries) == 18
    if which == "edges":
        n = entries[:, 0:3]
        assert (np.signbit(n) & (n == 0)).any() and (~np.signbit(n) & (n == 0)).any()  # both zeros occur
        assert (np.abs(n[:, 0]) == np.abs(n[:, 1]))[n[:, 0] != 0].any()               # the tie occurs


def test_table_normals_equal_the_reference_records():
    """For every hit record of a Rect, AABB or OBB in the reference's shapes_zoo fixture, the table's n for that shape and face
    (the face the host build of shape_surface_info reports for that ray) is the record's n."""
    from pine_amd import scenes
    z = np.load(os.path.join(GOLDEN, "shapes_zoo.npz"))
    rec, rays = z["records"], np.ascontiguousarray(z["rays"])
    sc = scenes.shapes_zoo((48, 48))
    assert sc.describe() == str(z["pscene"])
    entries, _, base, faces = frame_table(sc, rays=rays)
    assert faces.shape == rec.shape[:2] and len(base) == rec.shape[0]  # (the zoo has no mesh)
    checked = 0
    for g in range(len(base)):
        hit = rec[g, :, 1] == 1
        assert ((faces[g] >= 0) == (hit & (base[g] >= 0))).all(), g
        if base[g] < 0:
            continue
        assert_bit_equal(entries[base[g] + faces[g][hit], 0:3], rec[g][hit][:, 6:9], f"geometry {g}: table n vs reference n")
        assert hit.any(), f"the fixture has no hit record of geometry {g}"
        checked += 1
    assert checked == 4  # (the floor, the box, the transformed box, the lamp)


def test_scene_of_curved_shapes_has_no_table():
    import pine_amd as pa
    s = pa.Scene()
    s.add("d", pa.Diffuse([0.8, 0.8, 0.8]))
    s.add(pa.Sphere([0.5, 0.3, 1.2], 0.3), "d")
    s.add(pa.Disk([0.0, 1.5, 1.0], [0.2, -1.0, 0.1], 0.4), "d")
    s.add(pa.Cone([-0.3, 0.0, 1.4], [0, 1, 0], 0.2, 0.5), "d")
    s.add(pa.Cylinder([0, 0, 0], [0, 1, 0], 0.1), "d")
    s.add(pa.Sphere([0.0, 1.9, 1.0], 0.1), pa.Emissive([10.0, 10.0, 10.0]))
    s.set(pa.ThinLenCamera(pa.Film([16, 16]), [0, 1, -4], [0, 1, 0], 0.25))
    entries, _, base, _ = frame_table(s)
    assert len(entries) == 0 and (base == -1).all() and len(base) == 5


# ---- GPU ----

def _render(scene, spp, depth, **kw):
    """(film, stats, entries of the plan's table)."""
    import torch
    import pine_amd as pa
    w, h = scene.camera.film().size
    plan = pa.Plan(scene, spp, depth, **kw)
    film = torch.full((h, w, 4), -1.0, dtype=torch.float32, device="cuda")
    plan.launch(film.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    plan.check()
    st = plan.stats()
    n = len(frame_table(scene, plan)[0])
    out = film.cpu().numpy()
    plan.close()
    return out, st, n


FILMS = ["cbox_committed_64_s16_d4", "cbox_readme_64_s16_d4", "cbox_rect_readme_64_s64_d5", "mats_zoo_64_s32_d6", "zoo_48_s16_d5"]
CASES = [(k, n) for k in ("precompiled", "mega") for n in FILMS] + [("specialized", n) for n in FILMS[:3]]


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,name", CASES)
def test_films_with_the_table_are_the_golden_films(kernel, name, monkeypatch):
    """With the table, the film is the reference's, bit for bit; with $PINE_GPU_FRAME_TABLE=0 the same plan has no table, runs the
    same kernel and writes the same bytes."""
    ref, ps, spp, depth = load_film(name)
    sc = film_scene(name)
    assert sc.describe() == ps
    monkeypatch.delenv("PINE_GPU_FRAME_TABLE", raising=False)
    if kernel == "mega":
        monkeypatch.setenv("PINE_GPU_KERNEL", "mega")
    kw = {"specialize": kernel == "specialized"}
    film, st, n = _render(sc, spp, depth, **kw)
    flat = sum(FLAT_KINDS.get(k, 0) for k in kinds_of(sc))
    assert n == flat > 0, "the plan has no frame table"
    assert (st.specialized > 0) == (kernel == "specialized")
    assert_bit_equal(film, ref, f"{name}, {kernel} kernel, frame table")
    monkeypatch.setenv("PINE_GPU_FRAME_TABLE", "0")
    film0, st0, n0 = _render(sc, spp, depth, **kw)
    assert n0 == 0
    assert (st0.kernel_features, st0.specialized) == (st.kernel_features, st.specialized)
    assert film0.tobytes() == film.tobytes()


def lamp_among_spheres():
    """Curved shapes under one flat lamp: the only flat shape is emissive, and stage S never shades it."""
    import pine_amd as pa
    s = pa.Scene()
    s.add("d", pa.Diffuse([0.8, 0.8, 0.8]))
    s.add(pa.Sphere([0.0, -100.0, 1.0], 100.0), "d")
    s.add(pa.Sphere([0.3, 0.3, 1.2], 0.3), "d")
    s.add(pa.Cone([-0.4, 0.0, 1.4], [0, 1, 0], 0.2, 0.5), "d")
    s.add(pa.Rect([0.0, 1.9, 1], [0.5, 0, 0], [0, 0, 0.5]), pa.Emissive([20.0, 18.0, 15.0]))
    s.set(pa.ThinLenCamera(pa.Film([16, 16]), [0, 1, -4], [0, 1, 0], 0.25))
    return s


@pytest.mark.gpu
def test_plan_has_no_table_where_no_hit_would_read_it_from_lds(monkeypatch):
    """A plan keeps the table only where stage S can reach a flat shape and the kernel stages the blob in LDS.  A scene whose one
    flat shape is its lamp has a table of its own (the hook's host build) and a plan without one; a cbox plan pushed to a
    scene-in-global variant (the megakernel under $PINE_GPU_NO_LDS_SCENE) has none either.  Both write the films of their $PINE_GPU_FRAME_TABLE=0 twins."""
    from pine_amd import scenes
    monkeypatch.delenv("PINE_GPU_FRAME_TABLE", raising=False)
    s = lamp_among_spheres()
    assert len(frame_table(s)[0]) == 1
    film, st, entries = _render(s, 4, 3, specialize=False)
    assert entries == 0 and st.kernel_features & (1 << 8)  # (a scene-in-LDS variant: the rule, not the room, drops the table)
    c = scenes.cbox((32, 32))
    filmc, stc, entriesc = _render(c, 4, 3, specialize=False)
    assert entriesc == 18
    monkeypatch.setenv("PINE_GPU_NO_LDS_SCENE", "1")
    monkeypatch.setenv("PINE_GPU_KERNEL", "mega")
    filmg, stg, entriesg = _render(c, 4, 3, specialize=False)
    assert entriesg == 0 and not stg.kernel_features & ((1 << 8) | (1 << 14))
    assert filmg.tobytes() == filmc.tobytes()
    monkeypatch.delenv("PINE_GPU_NO_LDS_SCENE")
    monkeypatch.delenv("PINE_GPU_KERNEL")
    monkeypatch.setenv("PINE_GPU_FRAME_TABLE", "0")
    film0, st0, entries0 = _render(s, 4, 3, specialize=False)
    assert entries0 == 0 and (st0.kernel_features, st0.lds_bytes) == (st.kernel_features, st.lds_bytes)
    assert film0.tobytes() == film.tobytes()


def boxes_scene(n):
    import pine_amd as pa
    s = pa.Scene()
    s.add("d", pa.Diffuse([0.8, 0.8, 0.8]))
    s.add(pa.Rect([0, 0, 1], [2, 0, 0], [0, 0, 2], True), "d")
    for i in range(n):
        x, y = -0.9 + 0.2 * (i % 10), 0.05 + 0.2 * (i // 10)
        s.add(pa.Box([x, y, 1.0], [x + 0.15, y + 0.15, 1.15]), "d")
    s.add(pa.Rect([0.0, 1.9, 1], [0.5, 0, 0], [0, 0, 0.5]), pa.Emissive([20.0, 18.0, 15.0]))
    s.set(pa.ThinLenCamera(pa.Film([16, 16]), [0, 1, -4], [0, 1, 0], 0.25))
    return s


@pytest.mark.gpu
def test_plan_has_no_table_where_it_would_change_the_kernel(monkeypatch):
    """Scenes of 4 to 60 boxes: the table grows by 288 bytes per box, and somewhere on the way the scene's records still fit
    the LDS of a scene-in-LDS variant (F_LDS_SCENE, bit 8) while records and table together would not.  Every plan runs the
    kernel variant and has the LDS bytes of its $PINE_GPU_FRAME_TABLE=0 twin plus its table's, and writes the same film; the
    plan has either the whole table or none; and the range holds a scene with a table and a scene-in-LDS scene without."""
    kept, dropped_in_lds = 0, 0
    for n in range(4, 64, 4):
        s = boxes_scene(n)
        whole = len(frame_table(s)[0])
        assert whole == 6 * n + 2
        monkeypatch.delenv("PINE_GPU_FRAME_TABLE", raising=False)
        film, st, entries = _render(s, 4, 3, specialize=False)
        monkeypatch.setenv("PINE_GPU_FRAME_TABLE", "0")
        film0, st0, entries0 = _render(s, 4, 3, specialize=False)
        print(f"{n} boxes: kernel_features {st0.kernel_features:#x}, lds_bytes {st0.lds_bytes} -> {st.lds_bytes}, entries {entries} of {whole}")
        assert entries0 == 0 and entries in (0, whole), n
        assert st.kernel_features == st0.kernel_features, n
        table_bytes = (whole * 48 + (4 * (n + 2) + 15) // 16 * 16) if entries else 0
        assert st.lds_bytes in (st0.lds_bytes, st0.lds_bytes + table_bytes), n  # (a scene-in-global variant stages no table)
        assert film0.tobytes() == film.tobytes(), n
        kept += entries == whole
        dropped_in_lds += entries == 0 and bool(st0.kernel_features & (1 << 8))
    assert kept > 0 and dropped_in_lds > 0, (kept, dropped_in_lds)
